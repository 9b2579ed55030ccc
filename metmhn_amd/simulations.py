"""Gillespie sampling of the joint PT/MT process on the GPU - the reference's `metmhn/simulations.py` call
surface (`simulate_dat`, `simulate_orders`, :87-147) over `mmhn_simulate` (csrc/sampler.h), its reductions of
trajectories on the host (`extract_bse`, `preseeding_probs`, :150-240), and the same reductions counted on the
device without the samples (`simulate_summary`, `simulate_preseeding_probs` over `mmhn_simulate_summary`), and the
second-order counterpart: pairwise co-occurrence and burden tables (`simulate_pairs`, `PairSummary` over
`mmhn_simulate_pairs`) to hold a fit against the co-occurrence structure of its cohort.

`original_key` takes the place of the `jax.random.PRNGKey`: an int, or anything array-like whose integers are
folded into the 64-bit Philox key.  Streams differ from jax.random's; distributions do not."""
from __future__ import annotations

import numpy as np

from .engine import Engine
from .results import _residuals

_engines: dict = {}


def _engine(n_mut: int) -> Engine:
    from .engine import default_device
    key = (n_mut, default_device())
    if key not in _engines:
        _engines[key] = Engine(n_mut)
    return _engines[key]


def _seed(key) -> int:
    a = np.atleast_1d(np.asarray(key)).astype(np.uint64).ravel()
    s = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        for v in a:
            s = (s ^ v) * np.uint64(0xBF58476D1CE4E5B9)
            s ^= s >> np.uint64(31)
    return int(s)


def simulate_dat(log_theta, pt_d_ef, mt_d_ef, n_sim: int, original_key=0) -> np.ndarray:
    """int8 [n_sim, 2n+2]: genotypes `[PT_0, MT_0, ..., seeding]` + observation order (simulations.py:117-147)."""
    lt = np.asarray(log_theta, dtype=np.float64)
    return _engine(lt.shape[0] - 1).simulate(lt, pt_d_ef, mt_d_ef, n_sim, _seed(original_key))


def simulate_orders(log_theta, pt_d_ef, mt_d_ef, n_sim: int, original_key=0) -> np.ndarray:
    """int8 [n_sim, 2N+2]: event sequences padded with -99, events numbered as simulations.py:100-107."""
    lt = np.asarray(log_theta, dtype=np.float64)
    return _engine(lt.shape[0] - 1).simulate(lt, pt_d_ef, mt_d_ef, n_sim, _seed(original_key), orders=True)[1]


# ---- reductions of the samples (simulations.py:150-240, Utilityfunctions.py:116-155)

def extract_bse(traject, n: int, seeding_num: int):
    """Pre-seeding events and all events of trajectories as simulate_orders returns them (simulations.py:150-221).

    traject: int [2n+2] or [T, 2n+2], events numbered as simulate_orders numbers them, padded with -99.
    Returns int8 (bsc [.., n], tc [.., 2n+2]): bsc[e] = 1 if event e happened before the seeding (the seeding
    itself included), tc the events of the trajectory, pre-seeding events in both tumours (e and e + n + 1).
    Trajectories without the seeding give zeros.  Indices past the end of bsc / tc are dropped, as jax drops
    out-of-bounds scatters (a post-seeding event e >= n never clears bsc)."""
    t = np.asarray(traject)
    one = t.ndim == 1
    t = np.atleast_2d(t).astype(np.int64)
    T, L = t.shape
    bsc = np.zeros((T, n), dtype=np.int8)
    tc = np.zeros((T, 2 * n + 2), dtype=np.int8)
    rows = np.arange(T)
    live = np.any(t == seeding_num, axis=1)           # lax.cond: trajectories without the seeding stay zero
    pre = np.ones(T, dtype=bool)                       # psf: the seeding itself still counts as pre-seeding

    def put(arr, r, idx, v):
        ok = (idx >= 0) & (idx < arr.shape[1])
        arr[r[ok], idx[ok]] = v

    for i in range(L):
        e = t[:, i]
        live &= e != -99                               # the while loop ends at the first padding value
        pre_now, post_now = live & pre, live & ~pre
        put(bsc, rows[pre_now], e[pre_now], 1)
        put(tc, rows[pre_now], e[pre_now], 1)
        put(tc, rows[pre_now], e[pre_now] + n + 1, 1)
        put(bsc, rows[post_now], e[post_now], 0)
        put(tc, rows[post_now], e[post_now], 1)
        pre &= ~(live & (e == seeding_num))
    return (bsc[0], tc[0]) if one else (bsc, tc)


def preseeding_probs(dat, n: int, seeding_num: int):
    """(P(t_mut < t_seed | PT(mut) = 1, seeded), P(t_mut < t_seed | MT(mut) = 1, seeded)) from trajectories
    [T, 2n+2] as simulate_orders returns them (simulations.py:224-240); float64 [seeding_num] each, NaN where no
    seeded trajectory has the mutation (0 / 0)."""
    bsc, tc = extract_bse(np.atleast_2d(np.asarray(dat)), n, seeding_num)
    num = bsc[:, :-1].sum(axis=0, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pt_cond = num / tc[:, :seeding_num].sum(axis=0, dtype=np.int64)
        mt_cond = num / tc[:, seeding_num + 2:-2].sum(axis=0, dtype=np.int64)
    return pt_cond, mt_cond


class SimSummary:
    """Counts of Gillespie samples (mmhn_simulate_summary).  Totals n_sim, n_seeded, n_pt_first, n_mt_first; per
    mutation (int64 [n_mut]) over the seeded samples pre (occurred before the seeding), pt, mt, shared (final PT /
    MT / both bits) and over the unseeded ones pt_nm (final PT bit).  counts: the raw int64 vector."""

    def __init__(self, counts, n_mut: int):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.n_mut = n = int(n_mut)
        self.n_sim, self.n_seeded, self.n_pt_first, self.n_mt_first = (int(v) for v in self.counts[:4])
        self.pre, self.pt, self.mt, self.shared, self.pt_nm = (self.counts[4 + k * n:4 + (k + 1) * n] for k in range(5))

    def __repr__(self):
        return (f"SimSummary(n_mut={self.n_mut}, n_sim={self.n_sim}, n_seeded={self.n_seeded}, "
                f"n_pt_first={self.n_pt_first}, n_mt_first={self.n_mt_first})")

    def preseeding_probs(self):
        """preseeding_probs of the same samples: (pre / pt, pre / mt) in float64, NaN where the denominator is 0."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.pre / self.pt, self.pre / self.mt

    def marg_frequs(self, events, decimals: int = 2):
        """The model-implied counterpart of Utilityfunctions.marg_frequs: the seeded samples stand for the coupled,
        EM-PT and EM-MT rows, the unseeded ones for the NM rows; same layout, labels and rounding."""
        import pandas as pd
        s, u = self.n_seeded, self.n_sim - self.n_seeded
        seed_col = lambda c: np.append(c, 0)
        num = np.vstack((np.append(self.pt - self.shared, s), seed_col(self.mt - self.shared), seed_col(self.shared),
                         seed_col(self.pt_nm), np.append(self.pt, s), np.append(self.mt, s)))
        size = np.array([s, s, s, u, s, s], dtype=np.int64).reshape(-1, 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            tab = num / size
        labels = [[f"Coupled ({s})"] * 3 + [f"NM ({u})", f"EM-PT ({s})", f"EM-MT ({s})"],
                  ["PT-Private", "MT-Private", "Shared"] + ["Present"] * 3]
        inds = pd.MultiIndex.from_tuples(list(zip(*labels)))
        return pd.DataFrame(np.around(tab, decimals), columns=events, index=inds).T


def _check_params(log_theta, pt_d_ef, mt_d_ef):
    lt = np.asarray(log_theta, dtype=np.float64)
    if lt.ndim != 2 or lt.shape[0] != lt.shape[1] or lt.shape[0] < 2:
        raise ValueError(f"log_theta must have shape (N, N) with N >= 2, got {lt.shape}")
    N = lt.shape[0]
    for name, d in (("pt_d_ef", pt_d_ef), ("mt_d_ef", mt_d_ef)):
        if np.shape(d) != (N,):
            raise ValueError(f"{name} must have shape ({N},), got {np.shape(d)}")
    return lt


def simulate_summary(log_theta, pt_d_ef, mt_d_ef, n_sim: int, original_key=0, first: int = 0) -> SimSummary:
    """Counts of the samples [first, first + n_sim) on the GPU without materialising them (mmhn_simulate_summary).
    With first = 0 these are exactly the samples simulate_dat / simulate_orders(..., n_sim, original_key) return;
    n_sim is bounded by time, not memory, and `first` extends a run or splits it into parts with the same samples."""
    lt = _check_params(log_theta, pt_d_ef, mt_d_ef)
    if int(n_sim) < 0 or int(first) < 0:
        raise ValueError(f"n_sim and first must be non-negative, got n_sim={n_sim}, first={first}")
    n_mut = lt.shape[0] - 1
    counts = _engine(n_mut).simulate_summary(lt, pt_d_ef, mt_d_ef, int(n_sim), _seed(original_key), first=int(first))
    return SimSummary(counts, n_mut)


def simulate_preseeding_probs(log_theta, pt_d_ef, mt_d_ef, n_sim: int, original_key=0):
    """simulate_summary(...).preseeding_probs(): the pre-seeding probabilities of n_sim samples, counted on the GPU."""
    return simulate_summary(log_theta, pt_d_ef, mt_d_ef, n_sim, original_key).preseeding_probs()


# ---- second order: which events occur together (mmhn_simulate_pairs)

STRATA = ("NM", "EM-PT", "EM-MT", "paired")          # cohort row types 0 - 3, the strata of SimSummary.marg_frequs
BURDEN_KINDS = ("pt", "mt", "shared", "pt_private", "mt_private")


class PairSummary:
    """Pairwise co-occurrence and burden counts of Gillespie samples (mmhn_simulate_pairs), per class of sample: 0
    unseeded, 1 seeded and PT observed first, 2 seeded and MT observed first (simulate_dat's last column).

    n_class int64 [3]; pairs int64 [3, B, B], B = 2 n_mut: pairs[c] = G.T @ G over the class's rows of simulate_dat's
    genotype columns [PT_0, MT_0, PT_1, MT_1, ...] - symmetric, marginal counts on the diagonal, [2i, 2i+1] = event i in
    both tumours; burden int64 [3, 5, n_mut + 1]: histograms of |PT|, |MT|, |PT & MT|, |PT & ~MT|, |MT & ~PT|
    (BURDEN_KINDS).  The strata (STRATA) are what a cohort's row types observe: "NM" the PT columns of the unseeded
    samples, "EM-PT" / "EM-MT" the PT / MT columns of the seeded ones, "paired" all columns of the seeded ones."""

    def __init__(self, n_class, pairs, burden, n_mut: int):
        self.n_mut = n = int(n_mut)
        self.n_class = np.asarray(n_class, dtype=np.int64).reshape(3)
        self.pairs = np.asarray(pairs, dtype=np.int64).reshape(3, 2 * n, 2 * n)
        self.burden = np.asarray(burden, dtype=np.int64).reshape(3, 5, n + 1)

    def __repr__(self):
        return f"PairSummary(n_mut={self.n_mut}, n_class={self.n_class.tolist()})"

    def seeded(self):
        """(pairs[1] + pairs[2], n_class[1] + n_class[2]): the seeded samples, which a cohort's paired rows stand for."""
        return self.pairs[1] + self.pairs[2], int(self.n_class[1] + self.n_class[2])

    def _stratum(self, stratum):
        """(pair counts [B, B], samples, observed columns bool [B]) of a stratum."""
        if stratum not in STRATA:
            raise ValueError(f"stratum must be one of {STRATA}, got {stratum!r}")
        counts, n = (self.pairs[0], int(self.n_class[0])) if stratum == "NM" else self.seeded()
        is_pt = np.arange(2 * self.n_mut) % 2 == 0
        seen = {"NM": is_pt, "EM-PT": is_pt, "EM-MT": ~is_pt, "paired": np.ones_like(is_pt)}[stratum]
        return counts, n, seen

    def frequencies(self, stratum) -> np.ndarray:
        """pairs / samples of the stratum, float64 [B, B]: joint frequencies of two columns, marginal ones on the
        diagonal; NaN in the blocks the stratum does not observe (and everywhere if it has no sample)."""
        counts, n, seen = self._stratum(stratum)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = counts / np.float64(n)
        f[~(seen[:, None] & seen[None, :])] = np.nan
        return f

    def log_odds(self, stratum) -> np.ndarray:
        """Log odds ratio of every two columns from the stratum's 2x2 table: log(n11 n00 / (n10 n01)) with n11 the pair
        count and the other cells from the marginal counts; NaN where a cell is 0 (the diagonal included) and in the
        blocks the stratum does not observe."""
        counts, n, seen = self._stratum(stratum)
        m = np.diag(counts)
        n11 = counts.astype(np.float64)
        n10, n01 = m[:, None] - n11, m[None, :] - n11
        n00 = n - m[:, None] - m[None, :] + n11
        cells = np.stack((n11, n10, n01, n00))
        with np.errstate(divide="ignore", invalid="ignore"):
            lo = np.log(n11) + np.log(n00) - np.log(n10) - np.log(n01)
        lo[(cells <= 0).any(axis=0) | ~(seen[:, None] & seen[None, :])] = np.nan
        return lo

    def burden_pmf(self, kind, stratum) -> np.ndarray:
        """Normalised histogram [n_mut + 1] of a tumour's mutation count: kind 0 - 4 or its name in BURDEN_KINDS; "NM"
        and "EM-PT" observe |PT| only, "EM-MT" |MT| only, "paired" all five - NaN for a kind the stratum does not observe."""
        k = BURDEN_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        if not 0 <= k < 5:
            raise ValueError(f"kind must be 0 - 4 or one of {BURDEN_KINDS}, got {kind!r}")
        _, n, _ = self._stratum(stratum)
        if k not in {"NM": (0,), "EM-PT": (0,), "EM-MT": (1,), "paired": range(5)}[stratum]:
            return np.full(self.n_mut + 1, np.nan)
        h = self.burden[0, k] if stratum == "NM" else self.burden[1, k] + self.burden[2, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            return h / np.float64(n)

    def compare(self, dat) -> dict:
        """The posterior-predictive check of a cohort `dat` [n_pat, 2 n_mut + 3] (reference format, type in the last
        column): per row type present {stratum: residuals [B, B]}, the standardised residuals (obs - n p) / sqrt(n p (1 - p))
        of the observed pair counts (Utilityfunctions.pair_counts) against n = rows of the type and p = frequencies(stratum);
        NaN where p is 0, 1 or not observed by the type."""
        from .Utilityfunctions import pair_counts
        dat = np.asarray(dat)
        if dat.ndim != 2 or dat.shape[1] != 2 * self.n_mut + 3:
            raise ValueError(f"dat must have shape (n_pat, {2 * self.n_mut + 3}), got {dat.shape}")
        n_type, obs = pair_counts(dat)
        return {stratum: _residuals(obs[t], np.float64(n_type[t]), self.frequencies(stratum))
                for t, stratum in enumerate(STRATA) if n_type[t]}


def simulate_pairs(log_theta, pt_d_ef, mt_d_ef, n_sim: int, original_key=0, first: int = 0) -> PairSummary:
    """Pairwise co-occurrence and burden tables of the samples [first, first + n_sim) on the GPU without materialising
    them (mmhn_simulate_pairs); the samples are those of simulate_dat / simulate_summary under the same key."""
    lt = _check_params(log_theta, pt_d_ef, mt_d_ef)
    if int(n_sim) < 0 or int(first) < 0:
        raise ValueError(f"n_sim and first must be non-negative, got n_sim={n_sim}, first={first}")
    n_mut = lt.shape[0] - 1
    out = _engine(n_mut).simulate_pairs(lt, pt_d_ef, mt_d_ef, int(n_sim), _seed(original_key), first=int(first))
    return PairSummary(*out, n_mut)
