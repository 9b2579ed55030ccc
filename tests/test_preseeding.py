"""Reductions of simulated trajectories on the host (no GPU): `simulations.extract_bse` / `preseeding_probs` and
`Utilityfunctions.marg_frequs` against the reference's own functions (tests/golden/preseeding.npz, written by
tests/tools/make_golden_preseeding.py), and the argument checks of the summary sampler's wrappers, which must
raise before any engine exists."""
import numpy as np
import pandas as pd
import pytest

from metmhn_amd import Utilityfunctions as U
from metmhn_amd import simulations as S


@pytest.mark.parametrize("N", [4, 8])
def test_extract_bse_matches_reference(golden, N):
    g = golden("preseeding")
    traj = g[f"t{N}_traj"]
    bsc, tc = S.extract_bse(traj, N, N - 1)
    assert bsc.dtype == np.int8 and tc.dtype == np.int8
    np.testing.assert_array_equal(bsc, g[f"t{N}_bsc"])
    np.testing.assert_array_equal(tc, g[f"t{N}_tc"])
    for i in (0, 1, len(traj) - 1):                               # one trajectory at a time, as the reference takes it
        b, t = S.extract_bse(traj[i], N, N - 1)
        np.testing.assert_array_equal(b, g[f"t{N}_bsc"][i])
        np.testing.assert_array_equal(t, g[f"t{N}_tc"][i])


@pytest.mark.parametrize("N", [4, 8])
def test_preseeding_probs_match_reference(golden, N):
    g = golden("preseeding")
    traj = g[f"t{N}_traj"]
    pt, mt = S.preseeding_probs(traj, N, N - 1)
    assert pt.shape == mt.shape == (N - 1,) and pt.dtype == mt.dtype == np.float64
    np.testing.assert_array_equal(pt, g[f"t{N}_pt"])              # NaN positions included
    np.testing.assert_array_equal(mt, g[f"t{N}_mt"])
    unseeded = ~(traj == N - 1).any(axis=1)
    upt, umt = S.preseeding_probs(traj[unseeded], N, N - 1)
    assert np.isnan(g[f"t{N}_unseeded_pt"]).all()
    np.testing.assert_array_equal(upt, g[f"t{N}_unseeded_pt"])
    np.testing.assert_array_equal(umt, g[f"t{N}_unseeded_mt"])
    if N == 8:                                                     # mutation 5 never occurs: 0 / 0
        assert np.isnan(pt[5]) and np.isnan(mt[5]) and not np.isnan(np.delete(pt, 5)).any()


def test_marg_frequs_matches_reference(golden):
    g = golden("preseeding")
    events = [str(e) for e in g["mf_events"]]
    df = U.marg_frequs(g["mf_dat"], events)
    assert list(df.index) == events
    assert [list(c) for c in df.columns] == g["mf_cols"].tolist()
    np.testing.assert_array_equal(df.to_numpy(dtype=np.float64), g["mf_values"])


def test_marg_frequs_needs_every_type(golden):
    dat = golden("preseeding")["mf_dat"]
    events = [f"E{i}" for i in range((dat.shape[1] - 3) // 2)] + ["Seeding"]
    for t in range(4):
        with pytest.raises(ValueError, match="four types"):
            U.marg_frequs(dat[dat[:, -1] != t], events)


def test_summary_marg_frequs_layout():
    # n_mut = 2: 10 samples, 6 seeded (4 PT first); pre, pt, mt, shared, pt_nm per mutation
    counts = np.array([10, 6, 4, 2, 1, 0, 4, 3, 5, 2, 3, 0, 2, 1], dtype=np.int64)
    s = S.SimSummary(counts, 2)
    assert (s.n_sim, s.n_seeded, s.n_pt_first, s.n_mt_first) == (10, 6, 4, 2)
    pt, mt = s.preseeding_probs()
    np.testing.assert_array_equal(pt, [1 / 4, 0 / 3])
    np.testing.assert_array_equal(mt, [1 / 5, 0 / 2])
    df = s.marg_frequs(["A", "B", "Seeding"])
    exp = np.array([[1 / 6, 2 / 6, 3 / 6, 2 / 4, 4 / 6, 5 / 6],      # PT-only, MT-only, both; NM, EM-PT, EM-MT
                    [3 / 6, 2 / 6, 0 / 6, 1 / 4, 3 / 6, 2 / 6],
                    [1.0, 0.0, 0.0, 0.0, 1.0, 1.0]])
    np.testing.assert_array_equal(df.to_numpy(), np.around(exp, 2))
    assert list(df.columns) == [("Coupled (6)", "PT-Private"), ("Coupled (6)", "MT-Private"), ("Coupled (6)", "Shared"),
                                ("NM (4)", "Present"), ("EM-PT (6)", "Present"), ("EM-MT (6)", "Present")]
    empty = S.SimSummary(np.zeros(14, dtype=np.int64), 2)
    assert all(np.isnan(v).all() for v in empty.preseeding_probs())
    assert isinstance(empty.marg_frequs(["A", "B", "Seeding"]), pd.DataFrame)


def _never_called(*a, **k):
    raise AssertionError("an engine was created before the arguments were checked")


@pytest.mark.parametrize("case", ["theta", "theta_1d", "pt_d", "mt_d", "n_sim", "first"])
def test_summary_argument_checks(monkeypatch, case):
    monkeypatch.setattr(S, "_engine", _never_called)
    N = 4
    lt, dp, dm, n_sim, first = np.zeros((N, N)), np.zeros(N), np.zeros(N), 10, 0
    if case == "theta":
        lt = np.zeros((N, N + 1))
    elif case == "theta_1d":
        lt = np.zeros(N)
    elif case == "pt_d":
        dp = np.zeros(N - 1)
    elif case == "mt_d":
        dm = np.zeros((N, 1))
    elif case == "n_sim":
        n_sim = -1
    else:
        first = -5
    with pytest.raises(ValueError):
        S.simulate_summary(lt, dp, dm, n_sim, 0, first=first)
    if case not in ("first",):
        with pytest.raises(ValueError):
            S.simulate_preseeding_probs(lt, dp, dm, n_sim, 0)
