"""What the sampler tests share (test_montecarlo.py, test_simulate_summary.py, test_sampler_replay.py): the small model with
its NumPy-simulated patients, the datapoints whose frequency is compared with their probability, and the summary counts
formed on the host.  Imported by name; a module that imports the `sim` fixture gets a module-scoped instance of its own."""
import numpy as np
import pytest

N_SIM = 400_000


@pytest.fixture(scope="module")
def sim():
    from oracle import gillespie
    rng = np.random.default_rng(42)
    n_mut = 3
    lt = np.diag(rng.normal(size=n_mut + 1))
    off = rng.random((n_mut + 1, n_mut + 1)) < 0.3
    np.fill_diagonal(off, False)
    lt = lt + off * rng.normal(size=(n_mut + 1, n_mut + 1))
    dp = rng.normal(0, 1, size=n_mut + 1)
    dm = rng.normal(0, 1, size=n_mut + 1)
    dat = gillespie.simulate_dat(lt, dp, dm, N_SIM, seed=7)
    return lt, dp, dm, dat


def cases(dat):
    geno, order = dat[:, :-1], dat[:, -1]
    out = []

    def exact(g, sel=None):
        m = (geno == np.asarray(g, dtype=np.int8)).all(axis=1)
        return int((m if sel is None else m & sel).sum())
    # (dat row, simulated count) - rows as in test_likelihood.py
    out.append(("prim", [1] * 6 + [0, -99, 0], exact([1] * 6 + [0])))
    out.append(("prim_az", [0] * 6 + [0, -99, 0], exact([0] * 6 + [0])))
    pt_all = (geno[:, 0:6:2] == 1).all(axis=1) & (geno[:, 6] == 1)
    mt_all = (geno[:, 1:6:2] == 1).all(axis=1) & (geno[:, 6] == 1)
    out.append(("prim_met", [1] * 6 + [1, -99, 1], int(pt_all.sum())))
    out.append(("met", [1] * 6 + [1, -99, 2], int(mt_all.sum())))
    out.append(("coupled_0", [1] * 6 + [1, 0, 3], exact([1] * 7)))
    out.append(("coupled_1", [1] * 6 + [1, 1, 3], exact([1] * 7, order == 1)))
    out.append(("coupled_2", [1] * 6 + [1, 2, 3], exact([1] * 7, order == 2)))
    out.append(("empty", [0] * 6 + [1, 0, 3], exact([0] * 6 + [1])))
    out.append(("mixed_1", [1, 0, 1, 1, 0, 1, 1, 1, 3], exact([1, 0, 1, 1, 0, 1, 1], order == 1)))
    return out


def host_counts(d, od, n_mut):
    """The counts of include/metmhn_amd.h, from simulate_dat rows d and simulate_orders rows od."""
    from metmhn_amd import simulations as S
    N = n_mut + 1
    seeded = d[:, -2] == 1
    ptb, mtb = d[:, 0:2 * n_mut:2].astype(np.int64), d[:, 1:2 * n_mut:2].astype(np.int64)
    bsc, _ = S.extract_bse(od, N, N - 1)
    head = [len(d), seeded.sum(), (d[:, -1] == 1).sum(), (d[:, -1] == 2).sum()]
    rows = [bsc[:, :-1].sum(axis=0), ptb[seeded].sum(axis=0), mtb[seeded].sum(axis=0), (ptb & mtb)[seeded].sum(axis=0),
            ptb[~seeded].sum(axis=0)]
    return np.concatenate([np.array(head, dtype=np.int64)] + [r.astype(np.int64) for r in rows])
