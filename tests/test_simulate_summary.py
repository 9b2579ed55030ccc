"""The fused summary sampler (mmhn_simulate_summary, csrc/sampler.h k_gillespie_summary) on the GPU.

Its counts are pinned to the materialised sampler: with the same key it must describe exactly the samples
simulate_dat / simulate_orders return, counted on the host with the reference's reductions (extract_bse /
preseeding_probs / marg_frequs, themselves pinned to the reference by tests/test_preseeding.py).  Then chunking,
ranges, invariants, and a two-sample check against the NumPy sampler oracle/gillespie.py.
The exact check of both kernels against an independent replay of the stream is tests/test_sampler_replay.py."""
import numpy as np
import pandas as pd
import pytest

from metmhn_amd import Engine, synthetic
from metmhn_amd import Utilityfunctions as U
from metmhn_amd import simulations as S
from sampler_common import host_counts


def typed_cohort(d):
    """simulate_dat rows as a marg_frequs cohort: unseeded rows as NM (0); the seeded ones as coupled (3), EM-PT (1)
    and EM-MT (2) - the strata SimSummary.marg_frequs stands the seeded samples for."""
    s = d[d[:, -2] == 1]
    u = d[d[:, -2] == 0]
    col = lambda rows, t: np.hstack((rows, np.full((len(rows), 1), t, dtype=np.int8)))
    return np.vstack((col(u, 0), col(s, 3), col(s, 1), col(s, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("n_mut", [1, 3, 8, 20, 30])
@pytest.mark.parametrize("key", [0, 1234])
def test_summary_equals_materialised_samples(n_mut, key):
    lt, dp, dm = synthetic.random_params(n_mut)
    N, n_sim = n_mut + 1, 20_000
    d = S.simulate_dat(lt, dp, dm, n_sim, key)
    od = S.simulate_orders(lt, dp, dm, n_sim, key)
    summ = S.simulate_summary(lt, dp, dm, n_sim, key)
    exp = host_counts(d, od, n_mut)
    assert summ.counts.dtype == np.int64 and summ.counts.shape == (4 + 5 * n_mut,)
    np.testing.assert_array_equal(summ.counts, exp)
    assert 0 < summ.n_seeded < n_sim
    pt, mt = summ.preseeding_probs()
    rpt, rmt = S.preseeding_probs(od, N, N - 1)
    np.testing.assert_array_equal(pt, rpt)                         # bit-identical, NaNs in the same places
    np.testing.assert_array_equal(mt, rmt)
    np.testing.assert_array_equal(S.simulate_preseeding_probs(lt, dp, dm, n_sim, key)[0], rpt)
    events = [f"M{i}" for i in range(n_mut)] + ["Seeding"]
    pd.testing.assert_frame_equal(summ.marg_frequs(events), U.marg_frequs(typed_cohort(d), events))


@pytest.mark.gpu
def test_summary_chunking_and_ranges(monkeypatch):
    n_mut = 8
    lt, dp, dm = synthetic.random_params(n_mut)
    e = Engine(n_mut)
    ref = e.simulate_summary(lt, dp, dm, 5017, seed=9)
    monkeypatch.setenv("MMHN_SIM_CHUNK", "1000")
    small = Engine(n_mut)                                         # reads the switch when it is created
    np.testing.assert_array_equal(small.simulate_summary(lt, dp, dm, 5017, seed=9), ref)
    np.testing.assert_array_equal(small.simulate_summary(lt, dp, dm, 4321, seed=9, first=77),
                                  e.simulate_summary(lt, dp, dm, 4321, seed=9, first=77))
    a, b = 3001, 4999
    np.testing.assert_array_equal(e.simulate_summary(lt, dp, dm, a, seed=9) + e.simulate_summary(lt, dp, dm, b, seed=9, first=a),
                                  e.simulate_summary(lt, dp, dm, a + b, seed=9))
    hi = 2 ** 32 - 300                                            # the range crosses the counter's 32-bit word
    c1 = e.simulate_summary(lt, dp, dm, 1000, seed=9, first=hi)
    np.testing.assert_array_equal(c1, small.simulate_summary(lt, dp, dm, 1000, seed=9, first=hi))
    assert c1[0] == 1000 and (c1 != e.simulate_summary(lt, dp, dm, 1000, seed=9)).any()
    np.testing.assert_array_equal(e.simulate_summary(lt, dp, dm, 0, seed=9), np.zeros(4 + 5 * n_mut, dtype=np.int64))
    monkeypatch.delenv("MMHN_SIM_CHUNK")
    np.testing.assert_array_equal(Engine(n_mut, dtype="f32").simulate_summary(lt, dp, dm, 5017, seed=9), ref)
    with pytest.raises(ValueError):
        e.simulate_summary(lt, dp, dm, 10, seed=9, first=-1)
    with pytest.raises(RuntimeError, match="overflow"):
        e.simulate_summary(lt, dp, dm, 10, seed=9, first=2 ** 63 - 5)


@pytest.mark.gpu
@pytest.mark.parametrize("n_mut", [3, 20])
def test_summary_invariants_and_seeds(n_mut):
    lt, dp, dm = synthetic.random_params(n_mut)
    s1 = S.simulate_summary(lt, dp, dm, 100_000, 5)
    s2 = S.simulate_summary(lt, dp, dm, 100_000, 5)
    s3 = S.simulate_summary(lt, dp, dm, 100_000, 6)
    np.testing.assert_array_equal(s1.counts, s2.counts)
    assert (s1.counts != s3.counts).any()
    assert s1.n_sim == 100_000 and s1.n_pt_first + s1.n_mt_first == s1.n_seeded
    assert (s1.pre <= s1.shared).all() and (s1.shared <= np.minimum(s1.pt, s1.mt)).all()
    assert (s1.pt <= s1.n_seeded).all() and (s1.pt_nm <= s1.n_sim - s1.n_seeded).all()


@pytest.mark.gpu
def test_summary_matches_numpy_sampler():
    """Two-sample check against oracle/gillespie.py at 400 000 samples each: every frequency within 5 sigma."""
    from oracle import gillespie
    n_mut, n_sim = 6, 400_000
    lt, dp, dm = synthetic.random_params(n_mut)
    c = gillespie.simulate_dat(lt, dp, dm, n_sim, seed=11)
    s = S.simulate_summary(lt, dp, dm, n_sim, 3)
    seeded = c[:, -2] == 1
    ptb, mtb = c[:, 0:2 * n_mut:2].astype(np.int64), c[:, 1:2 * n_mut:2].astype(np.int64)
    pairs = [(s.n_seeded, seeded.sum()), (s.n_pt_first, (c[:, -1] == 1).sum()), (s.n_mt_first, (c[:, -1] == 2).sum())]
    pairs += list(zip(s.pt, ptb[seeded].sum(axis=0))) + list(zip(s.mt, mtb[seeded].sum(axis=0)))
    pairs += list(zip(s.shared, (ptb & mtb)[seeded].sum(axis=0))) + list(zip(s.pt_nm, ptb[~seeded].sum(axis=0)))
    worst = 0.0
    for x, y in pairs:
        x, y = int(x), int(y)
        if x + y < 200:
            continue
        p = (x + y) / (2 * n_sim)
        worst = max(worst, abs(x - y) / np.sqrt(2 * n_sim * p * (1 - p)))
    assert worst < 5.0, worst
