"""Pairwise co-occurrence and burden tables of simulated cohorts (mmhn_simulate_pairs, csrc/sampler.h k_gillespie_pairs;
simulations.simulate_pairs / PairSummary, Utilityfunctions.pair_counts).

The three arrays are defined by the rows simulate_dat returns for the same sample indices under the same key
(`definition` below restates include/metmhn_amd.h in NumPy), so every device check is an exact integer comparison: against
the definition at five sizes, against simulate_summary's marginals, at ragged sample counts, under chunking and index
ranges, and over more than two grid-stride passes of one launch.  The host side (pair_counts, PairSummary's methods, the
definition itself on the rows of oracle/sampler_replay.py) is checked without a device."""
import numpy as np
import pytest

from metmhn_amd import Engine, synthetic
from metmhn_amd import Utilityfunctions as U
from metmhn_amd import simulations as S

HIGH_KEY = 0x9E3779B97F4A7C15


def definition(d, n_mut):
    """(n_class [3], pairs [3, B, B], burden [3, 5, n_mut + 1]) of simulate_dat rows d."""
    B = 2 * n_mut
    G = d[:, :B].astype(np.int64)
    cls = d[:, -1]
    pt, mt = G[:, 0::2], G[:, 1::2]
    kinds = [pt.sum(1), mt.sum(1), (pt & mt).sum(1), (pt & (1 - mt)).sum(1), (mt & (1 - pt)).sum(1)]
    n_class = np.array([np.count_nonzero(cls == c) for c in range(3)], dtype=np.int64)
    pairs = np.stack([G[cls == c].T @ G[cls == c] for c in range(3)])
    burden = np.array([[np.bincount(k[cls == c], minlength=n_mut + 1) for k in kinds] for c in range(3)], dtype=np.int64)
    return n_class, pairs, burden


def assert_tables_equal(got, exp):
    for name, x, y in zip(("n_class", "pairs", "burden"), got, exp):
        assert x.dtype == np.int64 and x.shape == y.shape, name
        np.testing.assert_array_equal(x, y, err_msg=name)


# ---- on the device

@pytest.mark.gpu
@pytest.mark.parametrize("n_mut", [1, 2, 9, 20, 30])
@pytest.mark.parametrize("key", [0, HIGH_KEY])
def test_pairs_equal_materialised_samples(n_mut, key):
    """2 columns / 3 pairs, 10 pairs, the first shape with more than one pair per thread (171), the benchmark's shape
    (820) and the largest (60 columns, 1 830 pairs); 20 011 samples are no multiple of a wave or a workgroup."""
    lt, dp, dm = synthetic.random_params(n_mut)
    n_sim = 20_011
    d = S.simulate_dat(lt, dp, dm, n_sim, key)
    s = S.simulate_pairs(lt, dp, dm, n_sim, key)
    assert s.n_mut == n_mut
    assert_tables_equal((s.n_class, s.pairs, s.burden), definition(d, n_mut))
    for c in range(3):
        np.testing.assert_array_equal(s.pairs[c], s.pairs[c].T)
    assert s.n_class.sum() == n_sim and s.n_class[0] > 0 and s.n_class[1] + s.n_class[2] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_mut", [3, 20])
def test_pairs_consistent_with_summary(n_mut):
    lt, dp, dm = synthetic.random_params(n_mut)
    n_sim, key = 20_011, 17
    s = S.simulate_pairs(lt, dp, dm, n_sim, key)
    m = S.simulate_summary(lt, dp, dm, n_sim, key)
    seeded, n_seeded = s.seeded()
    ev, od = np.arange(0, 2 * n_mut, 2), np.arange(1, 2 * n_mut, 2)
    np.testing.assert_array_equal(np.diag(seeded)[ev], m.pt)
    np.testing.assert_array_equal(np.diag(seeded)[od], m.mt)
    np.testing.assert_array_equal(seeded[ev, od], m.shared)
    np.testing.assert_array_equal(np.diag(s.pairs[0])[ev], m.pt_nm)
    assert n_seeded == m.n_seeded and s.n_class.sum() == m.n_sim
    assert s.n_class[1] == m.n_pt_first and s.n_class[2] == m.n_mt_first and s.n_class[0] == m.n_sim - m.n_seeded
    np.testing.assert_array_equal(s.burden.sum(axis=2), np.repeat(s.n_class[:, None], 5, axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("n_sim", [0, 1, 63, 64, 65, 255, 256, 257])
def test_pairs_small_and_ragged(n_sim):
    """Waves with dead lanes and workgroups with dead waves count nothing for them; n_sim = 0 gives zeros."""
    n_mut = 9
    lt, dp, dm = synthetic.random_params(n_mut)
    e = Engine(n_mut)
    d = e.simulate(lt, dp, dm, n_sim, seed=21)
    got = e.simulate_pairs(lt, dp, dm, n_sim, seed=21)
    assert_tables_equal(got, definition(d, n_mut))
    assert got[0].sum() == n_sim


@pytest.mark.gpu
def test_pairs_chunking_and_ranges(monkeypatch):
    n_mut = 8
    lt, dp, dm = synthetic.random_params(n_mut)
    e = Engine(n_mut)
    ref = e.simulate_pairs(lt, dp, dm, 5017, seed=9)
    monkeypatch.setenv("MMHN_SIM_CHUNK", "1000")
    small = Engine(n_mut)                                         # reads the switch when it is created
    assert_tables_equal(small.simulate_pairs(lt, dp, dm, 5017, seed=9), ref)
    assert_tables_equal(small.simulate_pairs(lt, dp, dm, 4321, seed=9, first=77),
                        e.simulate_pairs(lt, dp, dm, 4321, seed=9, first=77))
    a, b = 3001, 4999
    parts = [x + y for x, y in zip(e.simulate_pairs(lt, dp, dm, a, seed=9), e.simulate_pairs(lt, dp, dm, b, seed=9, first=a))]
    assert_tables_equal(parts, e.simulate_pairs(lt, dp, dm, a + b, seed=9))
    hi = 2 ** 32 - 300                                            # the range crosses the counter's 32-bit word
    c1 = e.simulate_pairs(lt, dp, dm, 1000, seed=9, first=hi)
    assert_tables_equal(c1, small.simulate_pairs(lt, dp, dm, 1000, seed=9, first=hi))
    assert c1[0].sum() == 1000 and (c1[1] != e.simulate_pairs(lt, dp, dm, 1000, seed=9)[1]).any()
    monkeypatch.delenv("MMHN_SIM_CHUNK")
    assert_tables_equal(Engine(n_mut, dtype="f32").simulate_pairs(lt, dp, dm, 5017, seed=9), ref)
    with pytest.raises(ValueError):
        e.simulate_pairs(lt, dp, dm, 10, seed=9, first=-1)
    with pytest.raises(RuntimeError, match="overflow"):
        e.simulate_pairs(lt, dp, dm, 10, seed=9, first=2 ** 63 - 5)


@pytest.mark.gpu
def test_pairs_more_than_two_grid_stride_passes(monkeypatch):
    """One launch whose workgroups each make three passes (the last one ragged), against the definition and against the
    same samples in launches of 1 000."""
    import torch
    n_mut = 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_sim = 2 * 8 * cus * 256 + 777
    lt, dp, dm = synthetic.random_params(n_mut)
    e = Engine(n_mut)
    got = e.simulate_pairs(lt, dp, dm, n_sim, seed=4)
    assert_tables_equal(got, definition(e.simulate(lt, dp, dm, n_sim, seed=4), n_mut))
    monkeypatch.setenv("MMHN_SIM_CHUNK", "1000")
    assert_tables_equal(Engine(n_mut).simulate_pairs(lt, dp, dm, n_sim, seed=4), got)


@pytest.mark.gpu
def test_pairs_reproducible_and_keyed():
    lt, dp, dm = synthetic.random_params(9)
    s1, s2, s3 = (S.simulate_pairs(lt, dp, dm, 50_000, k) for k in (5, 5, 6))
    assert_tables_equal((s1.n_class, s1.pairs, s1.burden), (s2.n_class, s2.pairs, s2.burden))
    assert (s1.pairs != s3.pairs).any() and (s1.burden != s3.burden).any()


# ---- on the host

def small_cohort(n_mut=3, n_pat=90, seed=3):
    """A typed cohort in the reference's format: NM / EM-PT rows carry PT bits only, EM-MT rows MT bits only."""
    rng = np.random.default_rng(seed)
    dat = np.zeros((n_pat, 2 * n_mut + 3), dtype=np.int8)
    dat[:, :2 * n_mut] = rng.random((n_pat, 2 * n_mut)) < 0.4
    dat[:, -1] = rng.integers(0, 4, n_pat)
    dat[np.isin(dat[:, -1], (0, 1)), 1:2 * n_mut:2] = 0
    dat[dat[:, -1] == 2, 0:2 * n_mut:2] = 0
    dat[:, -3] = dat[:, -1] != 0
    return dat


def test_pair_counts_against_loops():
    n_mut = 3
    dat = small_cohort(n_mut)
    n_type, pairs = U.pair_counts(dat)
    assert n_type.dtype == np.int64 and pairs.dtype == np.int64 and pairs.shape == (4, 6, 6)
    exp_n, exp = np.zeros(4, dtype=np.int64), np.zeros((4, 6, 6), dtype=np.int64)
    for row in dat:
        exp_n[row[-1]] += 1
        for a in range(6):
            for b in range(6):
                exp[row[-1], a, b] += int(row[a]) * int(row[b])
    np.testing.assert_array_equal(n_type, exp_n)
    np.testing.assert_array_equal(pairs, exp)
    assert (n_type > 0).all()


def test_pair_summary_frequencies_and_nan_blocks():
    n_mut = 2
    rng = np.random.default_rng(0)
    pairs = rng.integers(1, 50, (3, 4, 4))
    pairs = pairs + pairs.transpose(0, 2, 1)
    s = S.PairSummary([200, 120, 80], pairs, np.zeros((3, 5, 3), dtype=np.int64), n_mut)
    seeded, n = s.seeded()
    np.testing.assert_array_equal(seeded, pairs[1] + pairs[2])
    assert n == 200
    pt, mt = np.array([0, 2]), np.array([1, 3])
    blocks = {"NM": (pairs[0] / 200, pt), "EM-PT": (seeded / 200, pt), "EM-MT": (seeded / 200, mt),
              "paired": (seeded / 200, np.arange(4))}
    for stratum, (exp, seen) in blocks.items():
        f = s.frequencies(stratum)
        assert f.dtype == np.float64 and f.shape == (4, 4)
        inside = np.zeros((4, 4), dtype=bool)
        inside[np.ix_(seen, seen)] = True
        np.testing.assert_array_equal(f[inside], exp[inside])
        assert np.isnan(f[~inside]).all() and not np.isnan(f[inside]).any()
    with pytest.raises(ValueError):
        s.frequencies("PT")


def test_pair_summary_log_odds_and_burden_pmf():
    # one mutation, 100 seeded samples: PT 50, MT 60, both 40 -> cells 40, 10, 20, 30 and an odds ratio of 6
    pairs = np.zeros((3, 2, 2), dtype=np.int64)
    pairs[1] = [[30, 25], [25, 35]]
    pairs[2] = [[20, 15], [15, 25]]
    burden = np.zeros((3, 5, 2), dtype=np.int64)
    burden[1, 0], burden[2, 0] = [30, 30], [20, 20]
    burden[0, 0] = [10, 30]
    s = S.PairSummary([40, 60, 40], pairs, burden, 1)
    lo = s.log_odds("paired")
    np.testing.assert_allclose(lo[0, 1], np.log(6.0), rtol=1e-14)   # four logs of a few ulps each
    np.testing.assert_allclose(lo[1, 0], np.log(6.0), rtol=1e-14)
    assert np.isnan(lo[0, 0]) and np.isnan(lo[1, 1])               # a column against itself has two empty cells
    assert np.isnan(s.log_odds("EM-PT")).all()                     # the only PT column, against itself
    np.testing.assert_array_equal(s.burden_pmf("pt", "paired"), [0.5, 0.5])
    np.testing.assert_array_equal(s.burden_pmf(0, "NM"), [0.25, 0.75])
    assert np.isnan(s.burden_pmf("mt", "EM-PT")).all()


def test_pair_summary_compare_residuals():
    """A model whose frequencies are the cohort's own gives residual 0 (up to the rounding of n * (obs / n) in float64);
    one more row without events moves n alone, and the residual follows its formula."""
    n_mut = 3
    dat = small_cohort(n_mut)
    dat = dat[np.isin(dat[:, -1], (0, 3))]                         # NM against class 0, paired against the seeded samples
    n_type, obs = U.pair_counts(dat)
    s = S.PairSummary([n_type[0], n_type[3], 0], np.stack((obs[0], obs[3], np.zeros_like(obs[0]))),
                      np.zeros((3, 5, n_mut + 1), dtype=np.int64), n_mut)
    res = s.compare(dat)
    assert set(res) == {"NM", "paired"}
    for stratum, t in (("NM", 0), ("paired", 3)):
        p = s.frequencies(stratum)
        inner = (p > 0) & (p < 1)
        assert inner.any() and np.isnan(res[stratum][~inner]).all()
        np.testing.assert_allclose(res[stratum][inner], 0.0, atol=1e-12)
    extra = np.zeros((1, dat.shape[1]), dtype=np.int8)
    extra[0, -1], extra[0, -3] = 3, 1                              # one more paired row without an event: n + 1, obs unchanged
    n, p = n_type[3] + 1, s.frequencies("paired")[0, 2]
    np.testing.assert_allclose(s.compare(np.vstack((dat, extra)))["paired"][0, 2],
                               (obs[3][0, 2] - n * p) / np.sqrt(n * p * (1 - p)), rtol=1e-12)


def test_definition_on_replayed_rows():
    """The host reference of the device tests, on the rows of the exact replay (oracle/sampler_replay.py): it runs, is
    symmetric, carries the marginals on its diagonal and every burden row sums to its class."""
    from oracle import sampler_replay
    n_mut = 4
    lt, dp, dm = synthetic.random_params(n_mut)
    d = sampler_replay.replay(lt, dp, dm, np.arange(600), 11).dat
    n_class, pairs, burden = definition(d, n_mut)
    assert n_class.sum() == 600 and (n_class > 0).all()
    for c in range(3):
        np.testing.assert_array_equal(pairs[c], pairs[c].T)
        np.testing.assert_array_equal(np.diag(pairs[c]), d[d[:, -1] == c][:, :2 * n_mut].astype(np.int64).sum(0))
        assert (pairs[c] <= np.minimum.outer(np.diag(pairs[c]), np.diag(pairs[c]))).all()
    np.testing.assert_array_equal(pairs[0][0::2, 0::2], pairs[0][1::2, 1::2])      # unseeded: the MT columns equal the PT ones
    np.testing.assert_array_equal(burden.sum(axis=2), np.repeat(n_class[:, None], 5, axis=1))
    assert (burden[0, 3:, 1:] == 0).all()                                             # and nothing is private there
    s = S.PairSummary(n_class, pairs, burden, n_mut)
    assert np.nanmax(s.frequencies("paired")) <= 1.0
