"""Order likelihoods and likeliest orders: the host-side mirror of metmhn/model.py (class MetMHN).

SURVEY.md §8 row f-4.  Same constructor, `likelihood(order, met_status, first_obs)` and
`likeliest_order(state, met_status, first_obs)` as the reference (model.py:184-376), same event
codes (2i = event i in the primary tumour, 2i+1 = event i in the metastasis, 2n = seeding; before
the seeding an event is written as the pair 2i, 2i+1), same error behaviour.

What runs where.  The diagonal of the restricted joint rate matrix, `_get_diag_paired`
(model.py:434-446 -> jx/kronvec.py kron_diag), is the device part and goes through the C ABI
(`mmhn_kron_diag`); without the HIP library it raises, there is no host substitute.  Everything
else in the reference's model.py is host code (NumPy/BLAS loops, dicts of candidate orders) and is
host code here.

How it differs from the reference inside.  A path's probability is a product of
"rate of this event / (observation rate + exit rate of the state it leads to)" factors.  With two
observations the first one may fall anywhere in the tail of the order, so a prefix carries a vector
    a   = probability of the prefix with no observation made yet,
    b_P = sum over admissible earlier "primary tumour observed here" points of the probability
          with the metastasis continuing on its own (model.py:1428-1538, 1540-1553),
    b_M = the same with the metastasis observed first (model.py:1555-1680),
and every later factor multiplies these by non-negative numbers.  `likelihood` walks one order with
that recurrence; `likeliest_order` runs it over the lattice of sub-states in index order and keeps,
per sub-state, only the candidates no other candidate dominates component-wise.  The reference keeps
EVERY order for seeded sub-states that do not yet hold all first-observed events
(model.py:574-619) and encodes orders as factorial-base int32 (k <= 12,
int_order_conversion.pyx:9); here the candidate lists stay short and orders are linked tuples, so
k is bounded by the 2^k lattice only.  Same maximum, same arg max when it is unique.
"""
from __future__ import annotations

import warnings
from types import SimpleNamespace

import numpy as np

from . import _philox
from .jx import kronvec as _kronvec
from .state import MetState, State

_FIRST_OBS = ("PT", "Met", "unknown", "sync")
_STATUS_ERR = "met_status must be one of 'isMetastasis', 'absent', 'present', 'isPaired'"
_FIRST_ERR = "first_obs must be one of 'PT', 'Met', 'unknown', 'sync'"
# a reference-format dat row -> likeliest_order's arguments (examples/post_training_analyses.ipynb): type dat[:, -1];
# first observation of a paired row dat[:, -2], 0 "unknown", 1 "PT" and any other value "Met" as the objective reads it
# (regularized_optimization.py:101-119)
_ROW_STATUS = {0: "absent", 1: "present", 2: "isMetastasis", 3: "isPaired"}
_ROW_FIRST = {0: "unknown", 1: "PT"}
# the reason codes of mmhn_likeliest_orders (MMHN_ORD_* of include/metmhn_amd.h) -> likeliest_order's messages
_ROW_ERRORS = {
    1: _STATUS_ERR,
    2: "This state is not reachable by mhn.",
    3: "a paired sample needs the seeding event",
    4: "PT part of the state was not empty, but met_status is 'isMetastasis'.",
    5: "Seeding was not observed, but met_status is 'isMetastasis'.",
    6: "Met part of the state was not empty, but met_status is 'absent'.",
    7: "Met part of the state was not empty, but met_status is 'present', not 'isPaired'.",
}


def _subset_sums(weights) -> np.ndarray:
    """out[x] = sum of weights[b] over the bits b of x."""
    out = np.zeros(1)
    for w in weights:
        out = np.concatenate((out, out + w))
    return out


def _subset_index(flags) -> np.ndarray:
    """out[x] = the bits of x whose flag is set, packed together (a software pext)."""
    out, nxt = np.zeros(1, dtype=np.int64), 0
    for f in flags:
        out = np.concatenate((out, out + (1 << nxt))) if f else np.concatenate((out, out))
        nxt += bool(f)
    return out


def _single_diag(theta: np.ndarray, n_events: int, events: list) -> np.ndarray:
    """Diagonal of a one-tumour rate matrix over `n_events` events, restricted to `events`:
    minus the summed rates of every event not yet present (model.py:378-432)."""
    diag = np.zeros(1 << len(events))
    for i in range(n_events):
        rate = np.exp(theta[i, i] + _subset_sums(theta[i, events]))
        if i in events:                       # already present in the upper half of its own bit
            rate[(np.arange(rate.size) >> events.index(i) & 1) == 1] = 0.0
        diag -= rate
    return diag


def _pareto(vecs: list) -> list:
    """Indices of the vectors no other vector dominates (>= everywhere, > somewhere); one of equals."""
    keep = []
    for i, v in enumerate(vecs):
        for j, w in enumerate(vecs):
            if j != i and all(wc >= vc for wc, vc in zip(w, v)) and (any(wc > vc for wc, vc in zip(w, v)) or j < i):
                break
        else:
            keep.append(i)
    return keep


class OrderPosterior(SimpleNamespace):
    """One observation summed over its admissible orders: log_evidence, pre [n], seed_pos [n+1]."""

    def __init__(self, log_evidence, pre, seed_pos):
        super().__init__(log_evidence=log_evidence, pre=pre, seed_pos=seed_pos)


class OrderPosteriors(OrderPosterior):
    """The same for every row of a cohort: log_evidence [n_pat], pre [n_pat, n], seed_pos [n_pat, n+1]."""

    def cohort_preseeding(self) -> np.ndarray:
        """Mean of `pre` over the rows that carry the seeding: the cohort's pre-seeding probabilities given the data
        (simulations.SimSummary.preseeding_probs is the same quantity of the model alone)."""
        seeded = ~np.isnan(self.pre).any(axis=1)
        return self.pre[seeded].mean(axis=0)


class OrderPrecedence(SimpleNamespace):
    """One observation summed over its admissible orders: log_evidence and prec [2n+1, 2n+1] over the event codes,
    prec[c, d] = P(c happened strictly earlier than d | the observation); NaN where a code is not in the observation."""

    def __init__(self, log_evidence, prec):
        super().__init__(log_evidence=log_evidence, prec=prec)


class OrderPrecedences(OrderPrecedence):
    """The same for every row of a cohort: log_evidence [n_pat], prec [n_pat, 2n+1, 2n+1]."""

    def cohort_mean(self) -> np.ndarray:
        """Entry by entry the mean of `prec` over the rows that carry both codes; NaN where no row does."""
        have = ~np.isnan(self.prec)
        rows = have.sum(axis=0)
        total = np.where(have, self.prec, 0.0).sum(axis=0)
        return np.where(rows > 0, total / np.maximum(rows, 1), np.nan)


class OrderPosition(SimpleNamespace):
    """One observation summed over its admissible orders: log_evidence, pos_pt and pos_mt [n+1, n+1] (event - n: the
    seeding -, position), pos[e, j] = P(e is the j-th (0-based) entry of that lineage | the observation).  The MT lineage
    of an order is the order without its even codes other than the seeding, the PT lineage the order without its odd
    codes.  NaN for an event the observation does not carry in the lineage (and throughout a lineage it does not have), 0
    at the positions past the lineage's length."""

    def __init__(self, log_evidence, pos_pt, pos_mt):
        super().__init__(log_evidence=log_evidence, pos_pt=pos_pt, pos_mt=pos_mt)


class OrderPositions(OrderPosition):
    """The same for every row of a cohort: log_evidence [n_pat], pos_pt and pos_mt [n_pat, n+1, n+1]."""

    def relative_profile(self, lineage: str = "mt", bins: int = None) -> np.ndarray:
        """Where in a lineage's history every event happens, over the cohort, on a common relative axis [n+1, bins]
        (examples/post_training_analyses.ipynb, "Finding relative event positions", with the posterior in the place of
        the likeliest order): a row whose lineage has L >= 1 entries adds pos[e, j] * L to the bins
        [bins * j // L, bins * (j + 1) // L) of every event e it carries, for every j < L.  `bins` defaults to
        lcm(1 ... the longest lineage), which every L divides - give it for lineages of more than a dozen entries, where that
        number is out of reach.  Rows without the lineage are skipped."""
        if lineage not in ("mt", "pt"):
            raise ValueError("lineage must be 'mt' or 'pt'")
        pos = self.pos_mt if lineage == "mt" else self.pos_pt
        carried = ~np.isnan(pos[:, :, 0])
        length = carried.sum(axis=1)
        if bins is None:
            bins = int(np.lcm.reduce(np.arange(1, max(int(length.max(initial=1)), 1) + 1)))
        out = np.zeros((pos.shape[1], bins))
        for i in np.flatnonzero(length > 0):
            L = int(length[i])
            for j in range(L):
                out[carried[i], bins * j // L:bins * (j + 1) // L] += pos[i, carried[i], j, None] * L
        return out


class OrderTime(SimpleNamespace):
    """One observation summed over its admissible orders and first-observation points: log_evidence, time [2n+1] over the
    event codes (the posterior mean of the time at which the code's event happened; NaN where the observation does not
    carry the code), obs [2] (the posterior mean time of the first and of the second observation; a one-tumour observation
    has (its observation, NaN)) and pt_first = P(the primary tumour was observed first | the observation), NaN for one
    tumour and for "sync".  Time 0 is the event-free state, the unit the one in which an event-free tumour is observed at
    rate 1."""

    def __init__(self, log_evidence, time, obs, pt_first):
        super().__init__(log_evidence=log_evidence, time=time, obs=obs, pt_first=pt_first)


class OrderTimes(OrderTime):
    """The same for every row of a cohort: log_evidence [n_pat], time [n_pat, 2n+1], obs [n_pat, 2], pt_first [n_pat]."""

    def relative(self, to: str = "last") -> np.ndarray:
        """[n_pat, 2n+1]: `time` over the row's last observation time (obs[:, 1] where the row has a second observation,
        obs[:, 0] elsewhere), or over its first (to="first").  A ratio of two expectations, NOT the expectation of the
        ratio: the posterior mean of (event time / observation time) is another number, which these arrays do not give."""
        if to not in ("first", "last"):
            raise ValueError("to must be 'first' or 'last'")
        first, second = self.obs[:, 0], self.obs[:, 1]
        scale = first if to == "first" else np.where(np.isnan(second), first, second)
        return self.time / scale[:, None]

    def cohort_mean(self, to: str = "last") -> np.ndarray:
        """[2n+1]: per event code the mean of relative(to) over the rows that carry the code; NaN where no row does."""
        rel = self.relative(to)
        have = ~np.isnan(rel)
        rows = have.sum(axis=0)
        total = np.where(have, rel, 0.0).sum(axis=0)
        return np.where(rows > 0, total / np.maximum(rows, 1), np.nan)


class OrderSnapshot(SimpleNamespace):
    """What the two tumours of one paired observation held at the moment of the first observation, summed over its
    admissible orders and first-observation points; r = 0: the primary tumour was observed first, r = 1: the metastasis.
    log_evidence; held [2, 2n+1] over the event codes, held[r, c] = P(the first observation was of tumour r and the event
    with code c had happened by then | the observation), NaN where the observation does not carry c, exactly 0 throughout
    the r that first_obs excludes; late [2, n+1], late[r, j] = P(the first observation was of tumour r and exactly j events of
    the other tumour happened after it | the observation); and the single most probable snapshot: map_first = its r,
    map_state [2n+1] (int8: 1 the code is held, 0 it is carried and still to come, -1 the observation does not carry it),
    map_prob its posterior probability.  An observation without a first observation - one tumour, or "sync" - has its
    log_evidence, NaN in held, late and map_prob and -1 in map_first and map_state."""

    def __init__(self, log_evidence, held, late, map_state, map_first, map_prob):
        super().__init__(log_evidence=log_evidence, held=held, late=late, map_state=map_state, map_first=map_first,
                         map_prob=map_prob)


class OrderSnapshots(OrderSnapshot):
    """The same for every row of a cohort: log_evidence [n_pat], held [n_pat, 2, 2n+1], late [n_pat, 2, n+1], map_state
    [n_pat, 2n+1] (int8), map_first [n_pat] (int32), map_prob [n_pat]."""

    def cohort_late(self) -> np.ndarray:
        """[n]: per mutation i the mean, over the paired rows that carry i in the later-observed tumour only, of the
        probability that i arose after the first observation.  A row that carries i in the metastasis and not in the
        primary tumour counts where the primary tumour can have been observed first (held[0, seeding] > 0: its diagnosis
        order is "PT" or "unknown"), with the term held[0, seeding] - held[0, 2i+1] = P(the primary tumour was observed first
        and i had not yet happened in the metastasis | the row); a row that carries i in the primary tumour only counts
        where the metastasis can have been observed first, with held[1, seeding] - held[1, 2i].  A term is divided by
        nothing: it is the joint probability of "this tumour was observed first" and "i came later", not the probability of
        the latter given the former, so an "unknown" row adds less than a row whose diagnosis order is known.  NaN where no
        row qualifies."""
        L = self.held.shape[-1]
        n = (L - 1) // 2
        have = ~np.isnan(self.held[:, 0, :])
        pt, mt = have[:, 0:2 * n:2], have[:, 1:2 * n:2]
        first = np.where(have[:, 2 * n, None], self.held[:, :, 2 * n], 0.0)          # [n_pat, 2]; 0: not a paired row
        after_pt = (mt & ~pt) & (first[:, 0, None] > 0.0)
        after_mt = (pt & ~mt) & (first[:, 1, None] > 0.0)
        term = (np.where(after_pt, first[:, 0, None] - self.held[:, 0, 1:2 * n:2], 0.0)
                + np.where(after_mt, first[:, 1, None] - self.held[:, 1, 0:2 * n:2], 0.0))
        rows = (after_pt | after_mt).sum(axis=0)
        return np.where(rows > 0, term.sum(axis=0) / np.maximum(rows, 1), np.nan)


class OrderSample(SimpleNamespace):
    """Orders of one observation drawn from its exact posterior: log_evidence, orders [n_samples, 2n+1] (int8 event codes
    of likeliest_order, padded with -1), log_prob [n_samples] = log P(order | the observation), margin [n_samples] = the
    smallest |u total - cumulative boundary| / total over the sample's moves (how far its draws stayed from every
    boundary: a last-bit difference of a weight cannot change a sample whose margin is larger than that difference), and
    totals [n_samples, moves] = the summed candidate weights of every move (NaN past the sample's last move)."""

    def __init__(self, log_evidence, orders, log_prob, margin, totals=None):
        super().__init__(log_evidence=log_evidence, orders=orders, log_prob=log_prob, margin=margin, totals=totals)


def _entry_times(orders: np.ndarray):
    """Of sampled orders [..., L] (event codes padded with -1): the codes as int64, whether an order holds the seeding,
    the seeding's index, and which entries are the second code of a joint event (2i, 2i+1 written next to each other
    before the seeding: both happen at the moment of the first)."""
    o = orders.astype(np.int64)
    L = o.shape[-1]
    pos = np.arange(L)
    is_seed = o == L - 1
    seeded = is_seed.any(axis=-1)
    sp = np.where(seeded, is_seed.argmax(axis=-1), 0)
    second = np.zeros(o.shape, dtype=bool)
    second[..., 1:] = (o[..., 1:] == o[..., :-1] + 1) & (o[..., :-1] % 2 == 0) & (pos[1:] < sp[..., None])
    return o, seeded, sp, second


class OrderSamples(SimpleNamespace):
    """Orders of every row of a cohort drawn from the rows' exact posteriors: log_evidence [n_pat], orders
    [n_pat, n_samples, 2n+1] (int8, padded with -1), log_prob [n_pat, n_samples]."""

    def __init__(self, log_evidence, orders, log_prob):
        super().__init__(log_evidence=log_evidence, orders=orders, log_prob=log_prob)

    def preseeding(self, rows_per_step: int = 256) -> np.ndarray:
        """[n_pat, n]: the share of a row's samples in which mutation m occurred before the seeding - the sample mean
        that estimates order_posteriors().pre; NaN in the rows without the seeding (and without samples)."""
        P, S, L = self.orders.shape
        n = (L - 1) // 2
        out = np.full((P, n), np.nan)
        if S == 0:
            return out
        pos = np.arange(L)
        for lo in range(0, P, rows_per_step):
            o, seeded, sp, second = _entry_times(self.orders[lo:lo + rows_per_step])
            R = o.shape[0]
            count = (pos < sp[..., None]) & ~second & (o >= 0)            # an event before the seeding, counted once
            idx = (np.arange(R)[:, None, None] * n + (o >> 1))[count]
            share = np.bincount(idx, minlength=R * n).reshape(R, n) / S
            out[lo:lo + R] = np.where(seeded[:, :1], share, np.nan)
        return out

    def precedence(self) -> np.ndarray:
        """[n_pat, 2n+1, 2n+1]: the share of a row's samples in which code c happened strictly earlier than code d - the
        sample mean that estimates order_precedences().prec (the two codes of a joint event before the seeding happen at
        the same moment); NaN where a code is not in the row."""
        P, S, L = self.orders.shape
        out = np.full((P, L, L), np.nan)
        if S == 0:
            return out
        pos, rows = np.arange(L), np.arange(S)[:, None]
        for p in range(P):
            o, _, _, second = _entry_times(self.orders[p])
            k = int((o[0] >= 0).sum())
            if k == 0:
                continue
            t = np.broadcast_to(pos, (S, L)) - second                     # the moment of every entry
            when = np.zeros((S, L), dtype=np.int64)
            when[rows, o[:, :k]] = t[:, :k]                               # ... and of every code
            codes = np.sort(o[0, :k])
            w = when[:, codes]
            out[p][np.ix_(codes, codes)] = (w[:, :, None] < w[:, None, :]).mean(axis=0)
        return out


class SeedingForecast(SimpleNamespace):
    """What lies ahead of a primary tumour that holds a genotype and has not seeded, until the seeding (or the model's own
    clock of the first observation, whichever comes first): `p_seed` = P(the seeding comes before the clock), 1 until the
    seeding; `time` = the expected time until then (order_time's unit); `before[j]` = P(mutation j arises before then);
    `with_seed[j]` = P(the seeding comes first and the seeding cell carries j) - both [n], NaN for a mutation the genotype
    holds; `n_before[m]` = P(the seeding comes first, after exactly m new mutations) [n+1]; `next[j]` = P(the next event is
    mutation j), next[n] the seeding [n+1], NaN for a held mutation.  No reference counterpart."""

    def __init__(self, p_seed, time, before, with_seed, n_before, next):
        super().__init__(p_seed=p_seed, time=time, before=before, with_seed=with_seed, n_before=n_before, next=next)


class SeedingForecasts(SeedingForecast):
    """SeedingForecast of R genotypes: every field with a leading axis over the rows."""

    def expected_new_events(self) -> np.ndarray:
        """The expected number of new mutations before the seeding (or the clock) [R]: the sum of `before` over the free
        mutations."""
        return np.nansum(self.before, axis=1)


class SeedingLandscape(SimpleNamespace):
    """The four forecast scalars of many genotypes of one model, arrays over the genotypes `codes` (bit j of a code =
    mutation j held): `p_seed`, `time` as SeedingForecast has them, `new_events` = the expected number of new mutations before
    the seeding or the clock (SeedingForecasts.expected_new_events()), `seed_events` = the expected number of new mutations
    the seeding cell carries where the seeding comes first (the sum of with_seed).  MetMHN.seeding_landscape returns every
    genotype, codes = 0 .. 2^n - 1; seeding_landscape_at the rows it was given.  No reference counterpart."""

    FIELDS = ("p_seed", "time", "new_events", "seed_events")

    def __init__(self, p_seed, time, new_events, seed_events, codes):
        super().__init__(p_seed=p_seed, time=time, new_events=new_events, seed_events=seed_events, codes=codes)

    def neighbours(self, genotype) -> np.ndarray:
        """[n + 1, 4]: the four values of `genotype` (n entries 0 / 1) in row 0 and, in row 1 + j, of the genotype one
        mutation j further - NaN where the genotype holds j already.  A lookup on a full landscape."""
        size = len(self.codes)
        n = size.bit_length() - 1
        if size != 1 << n or not np.array_equal(self.codes, np.arange(size)):
            raise ValueError("neighbours needs a full landscape (MetMHN.seeding_landscape)")
        g = np.asarray(genotype)
        if g.shape != (n,) or not np.isin(g, (0, 1)).all():
            raise ValueError(f"genotype must have {n} entries 0 / 1")
        x = int(sum(1 << j for j in range(n) if g[j]))
        at = lambda code: [float(getattr(self, name)[code]) for name in self.FIELDS]
        out = np.full((n + 1, 4), np.nan)
        out[0] = at(x)
        for j in range(n):
            if not g[j]:
                out[1 + j] = at(x | 1 << j)
        return out


GENOTYPE_STRATA = ("NM", "EM-PT", "unknown")     # cohort row types 0, 1 and 4: what is known of the seeding when a PT is observed


class GenotypeSummary:
    """Exact sums over the genotype distribution of the primary tumour, per plane s (0: observed unseeded, 1: observed
    seeded): mass [2] = sum_x P_s(x), pairs [2, n, n] = sum_x P_s(x) x_i x_j with the marginals on the diagonal, burden
    [2, n+1] = sum over |x| = m of P_s(x).  The interface of simulations.PairSummary restricted to the primary tumour -
    what simulate_pairs estimates from samples, without the sampling error.  Strata (GENOTYPE_STRATA): "NM" plane 0 over
    mass[0], "EM-PT" plane 1 over mass[1], "unknown" the sum of both planes (over mass[0] + mass[1] = 1)."""

    def __init__(self, mass, pairs, burden):
        self.mass = np.asarray(mass, dtype=np.float64).reshape(2)
        self.burden = np.asarray(burden, dtype=np.float64)
        self.n_mut = n = self.burden.shape[-1] - 1
        self.burden = self.burden.reshape(2, n + 1)
        self.pairs = np.asarray(pairs, dtype=np.float64).reshape(2, n, n)

    def __repr__(self):
        return f"GenotypeSummary(n_mut={self.n_mut}, mass={self.mass.tolist()})"

    def _stratum(self, stratum):
        """(pair sums [n, n], burden sums [n+1], mass) of a stratum."""
        if stratum not in GENOTYPE_STRATA:
            raise ValueError(f"stratum must be one of {GENOTYPE_STRATA}, got {stratum!r}")
        if stratum == "unknown":
            return self.pairs[0] + self.pairs[1], self.burden[0] + self.burden[1], self.mass[0] + self.mass[1]
        s = GENOTYPE_STRATA.index(stratum)
        return self.pairs[s], self.burden[s], self.mass[s]

    def frequencies(self, stratum) -> np.ndarray:
        """pairs / mass of the stratum, float64 [n, n]: joint frequencies of two mutations, marginal ones on the diagonal
        (NaN everywhere if the stratum has no mass)."""
        pairs, _, mass = self._stratum(stratum)
        with np.errstate(divide="ignore", invalid="ignore"):
            return pairs / np.float64(mass)

    def log_odds(self, stratum) -> np.ndarray:
        """Log odds ratio of every two mutations from the stratum's 2x2 table: log(p11 p00 / (p10 p01)) with p11 the pair
        frequency and the other cells from the marginal ones; NaN where a cell is not positive (the diagonal included)."""
        f = self.frequencies(stratum)
        m = np.diag(f)
        p10, p01 = m[:, None] - f, m[None, :] - f
        p00 = 1.0 - m[:, None] - m[None, :] + f
        cells = np.stack((f, p10, p01, p00))
        with np.errstate(divide="ignore", invalid="ignore"):
            lo = np.log(f) + np.log(p00) - np.log(p10) - np.log(p01)
        lo[~(cells > 0).all(axis=0)] = np.nan
        return lo

    def burden_pmf(self, stratum) -> np.ndarray:
        """burden / mass of the stratum [n+1]: the distribution of the primary tumour's mutation count."""
        _, burden, mass = self._stratum(stratum)
        with np.errstate(divide="ignore", invalid="ignore"):
            return burden / np.float64(mass)

    def compare(self, dat) -> dict:
        """The check of a cohort `dat` [n_pat, 2 n_mut + 3] (reference format, type in the last column) against the exact
        frequencies: per row type present among 0, 1 and 4 {stratum: residuals [n, n]}, the standardised residuals
        (obs - n p) / sqrt(n p (1 - p)) of the observed PT pair counts of the type's rows against n = rows of the type and
        p = frequencies(stratum) - simulations.PairSummary.compare's formula; NaN where p is not inside (0, 1).  Type 4 is
        counted from `dat` directly (Utilityfunctions.pair_counts ignores it)."""
        from .Utilityfunctions import pair_counts
        dat = np.asarray(dat)
        n = self.n_mut
        if dat.ndim != 2 or dat.shape[1] != 2 * n + 3:
            raise ValueError(f"dat must have shape (n_pat, {2 * n + 3}), got {dat.shape}")
        n_type, obs = pair_counts(dat)
        g4 = dat[dat[:, -1] == 4][:, 0:2 * n:2].astype(np.int64)
        seen = {"NM": (int(n_type[0]), obs[0][0::2, 0::2]), "EM-PT": (int(n_type[1]), obs[1][0::2, 0::2]),
                "unknown": (g4.shape[0], g4.T @ g4)}
        out = {}
        for stratum in GENOTYPE_STRATA:
            rows, counts = seen[stratum]
            if rows == 0:
                continue
            p = self.frequencies(stratum)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = (counts - rows * p) / np.sqrt(rows * p * (1.0 - p))
            r[~((p > 0.0) & (p < 1.0))] = np.nan
            out[stratum] = r
        return out


class GenotypeDistribution(SimpleNamespace):
    """The probability that the primary tumour is observed with a genotype and has not seeded (`unseeded`, the likelihood
    of the cohort row of type 0) or has seeded by then (`seeded`, type 1), arrays over the genotypes `codes` (bit j of a
    code = mutation j held), with `summary`, the GenotypeSummary of the WHOLE lattice.  MetMHN.genotype_distribution
    returns every genotype, codes = 0 .. 2^n - 1; genotype_distribution_at the rows it was given."""

    def __init__(self, unseeded, seeded, codes, summary):
        super().__init__(unseeded=unseeded, seeded=seeded, codes=codes, summary=summary)

    @property
    def total(self) -> np.ndarray:
        """unseeded + seeded: the likelihood of the row of unknown status (type 4)."""
        return self.unseeded + self.seeded

    @property
    def p_seeded(self) -> np.ndarray:
        """seeded / total: P(seeded | genotype), met_status_posterior's value (NaN where total is 0)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.seeded / self.total


METASTASIS_STRATA = ("founder", "MT")           # the planes of the metastasis distribution's summary


class MetastasisSummary(GenotypeSummary):
    """Exact sums over the genotype distribution of the metastasis' founder (plane 0: the genotype of the cell that seeds,
    Z) and of the metastasis at its observation (plane 1, M), GenotypeSummary's arrays: mass [2] (the two are equal, the
    probability that the seeding happens before the primary tumour's observation), pairs [2, n, n], burden [2, n+1].  Strata
    (METASTASIS_STRATA): "founder" plane 0 over mass[0], "MT" plane 1 over mass[1]; frequencies, log_odds and burden_pmf are
    GenotypeSummary's."""

    def __repr__(self):
        return f"MetastasisSummary(n_mut={self.n_mut}, mass={self.mass.tolist()})"

    def _stratum(self, stratum):
        if stratum not in METASTASIS_STRATA:
            raise ValueError(f"stratum must be one of {METASTASIS_STRATA}, got {stratum!r}")
        s = METASTASIS_STRATA.index(stratum)
        return self.pairs[s], self.burden[s], self.mass[s]

    def acquired(self) -> np.ndarray:
        """[n]: the probability that the metastasis gained mutation j after the seeding - the marginal frequency of j in
        the metastasis minus the one in its founder (the founder's mutations all stay)."""
        return np.diag(self.frequencies("MT")) - np.diag(self.frequencies("founder"))

    def expected_founder_events(self) -> float:
        """The expected number of mutations the seeding cell holds: sum_m m burden_pmf("founder")[m]."""
        return float(np.arange(self.n_mut + 1) @ self.burden_pmf("founder"))

    def compare(self, dat) -> dict:
        """The check of a cohort `dat` [n_pat, 2 n_mut + 3] against the exact frequencies of the metastasis: per row type
        present among 2 (key "EM-MT") and 3 (key "paired") the standardised residuals [n, n]
        (obs - rows p) / sqrt(rows p (1 - p)) of the observed MT-block pair counts of the type's rows
        (Utilityfunctions.pair_counts(dat)[1][t][1::2, 1::2]) against p = frequencies("MT") - simulations.PairSummary.compare's
        formula; NaN where p is not inside (0, 1)."""
        from .Utilityfunctions import pair_counts
        dat = np.asarray(dat)
        n = self.n_mut
        if dat.ndim != 2 or dat.shape[1] != 2 * n + 3:
            raise ValueError(f"dat must have shape (n_pat, {2 * n + 3}), got {dat.shape}")
        n_type, obs = pair_counts(dat)
        p = self.frequencies("MT")
        out = {}
        for key, t in (("EM-MT", 2), ("paired", 3)):
            rows = int(n_type[t])
            if rows == 0:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                r = (obs[t][1::2, 1::2] - rows * p) / np.sqrt(rows * p * (1.0 - p))
            r[~((p > 0.0) & (p < 1.0))] = np.nan
            out[key] = r
        return out


class MetastasisDistribution(SimpleNamespace):
    """The probability that the seeding happens before the primary tumour's observation and the seeding cell holds exactly
    a genotype (`founder`, Z), that the metastasis is observed with it (`metastasis`, M, the likelihood of the cohort row of
    type 2) and M weighted by how many of the genotype's mutations the founder held (`founder_weighted`, C), arrays over
    the genotypes `codes` (bit j of a code = mutation j held), with `summary`, the MetastasisSummary of the WHOLE lattice.
    MetMHN.metastasis_distribution returns every genotype, codes = 0 .. 2^n - 1; metastasis_distribution_at the rows it
    was given."""

    def __init__(self, founder, metastasis, founder_weighted, codes, summary):
        super().__init__(founder=founder, metastasis=metastasis, founder_weighted=founder_weighted, codes=codes,
                         summary=summary)

    @property
    def founder_events(self) -> np.ndarray:
        """founder_weighted / metastasis: the expected number of the metastasis' mutations that were already in the
        founder, given only the MT genotype (NaN where metastasis is 0)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            out = self.founder_weighted / self.metastasis
        return np.where(self.metastasis == 0, np.nan, out)


PARTNER_STRATA = ("founder", "partner")         # the planes of a partner distribution's summary
_PARTNER_GIVEN = ("PT", "MT")


class PartnerSummary(GenotypeSummary):
    """Exact sums over the joint distribution of one observed tumour with the founder (plane 0, W) and with the tumour
    that was not sequenced, the partner (plane 1, J), GenotypeSummary's arrays: mass [2] (the two are equal, the
    probability of the observed tumour's genotype), pairs [2, n, n], burden [2, n+1] - unnormalised, as in the siblings.
    Strata (PARTNER_STRATA): "founder" plane 0 over mass[0], "partner" plane 1 over mass[1]; frequencies, log_odds and
    burden_pmf are GenotypeSummary's and divide by the stratum's mass, so they are conditional on the observed tumour."""

    def __repr__(self):
        return f"PartnerSummary(n_mut={self.n_mut}, mass={self.mass.tolist()})"

    def _stratum(self, stratum):
        if stratum not in PARTNER_STRATA:
            raise ValueError(f"stratum must be one of {PARTNER_STRATA}, got {stratum!r}")
        s = PARTNER_STRATA.index(stratum)
        return self.pairs[s], self.burden[s], self.mass[s]

    def conditional_frequencies(self, stratum="partner") -> np.ndarray:
        """[n]: the probability that the stratum's genotype holds mutation j given the observed tumour - the marginal sums
        over the stratum's mass (NaN throughout if the mass is 0)."""
        pairs, _, mass = self._stratum(stratum)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(pairs) / np.float64(mass)

    def expected_burden(self, stratum="partner") -> float:
        """The expected number of mutations of the stratum's genotype given the observed tumour."""
        return float(np.arange(self.n_mut + 1) @ self.burden_pmf(stratum))

    def _held(self, genotype):
        g = np.asarray(genotype)
        if g.shape != (self.n_mut,) or not np.isin(g, (0, 1)).all():
            raise ValueError(f"genotype must be {self.n_mut} entries of 0 / 1")
        return g.astype(bool)

    def gained(self, genotype) -> np.ndarray:
        """[n]: the conditional probability that the partner holds mutation j, for the mutations the observed `genotype`
        lacks (NaN for the ones it holds)."""
        return np.where(self._held(genotype), np.nan, self.conditional_frequencies("partner"))

    def lost(self, genotype) -> np.ndarray:
        """[n]: the conditional probability that the partner lacks mutation j, for the mutations the observed `genotype`
        holds (NaN for the ones it lacks)."""
        return np.where(self._held(genotype), 1.0 - self.conditional_frequencies("partner"), np.nan)


class PartnerDistribution(SimpleNamespace):
    """The joint probability of one observed tumour - the primary tumour seeded (`given` "PT") or the metastasis ("MT")
    with the genotype `genotype` (a code) - with every founder genotype (`founder`, W) and with every genotype of the
    other tumour (`partner`, J: exp(lp) of the paired row of unknown order), arrays over the genotypes `codes`; `mass`
    their common sum, the probability of the observed tumour; `summary` the PartnerSummary."""

    def __init__(self, founder, partner, codes, mass, summary, given, genotype):
        super().__init__(founder=founder, partner=partner, codes=codes, mass=mass, summary=summary, given=given,
                         genotype=genotype)

    @property
    def conditional(self) -> np.ndarray:
        """partner / mass: the distribution of the other tumour's genotype given the observed one (NaN if mass is 0)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.partner / np.float64(self.mass)

    @property
    def founder_conditional(self) -> np.ndarray:
        """founder / mass: the distribution of the founder's genotype given the observed tumour (NaN if mass is 0)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.founder / np.float64(self.mass)


_FORECAST_UNTIL = ("seeding", "observation")
_FORECAST_HOST_MAX = 24          # free mutations the host definition takes on: f x 2^f doubles of rates
_LATTICE_HOST_MAX = 24           # mutations the host landscape and distributions take on: n x 2^n doubles of rates
_NO_SEEDING_EXIT = ("the seeding rate of the full genotype underflows to 0 (a theta[n, n] of -1e10, as a fit without seeded "
                    "samples leaves it?): until='seeding' the full state would have no exit; use until='observation'")


class MetMHN:
    """The metastasis MHN with its two observation-rate vectors (model.py:175-211)."""

    def __init__(self, log_theta, obs1, obs2, events: list = None, meta: dict = None):
        self.log_theta = np.array(log_theta, dtype=np.float64)
        self.obs1 = np.array(obs1, dtype=np.float64)
        self.obs2 = np.array(obs2, dtype=np.float64)
        self.events = events
        self.meta = meta
        self.n = self.log_theta.shape[1] - 1
        # the primary tumour does not feel the seeding (model.py:207-208)
        self._pt_log_theta = self.log_theta.copy()
        self._pt_log_theta[:-1, -1] = 0.0
        self.orders_fallback_rows = 0       # rows the last likeliest_orders call recomputed on the host
        self.posteriors_fallback_rows = 0   # ... and the last order_posteriors call
        self.precedences_fallback_rows = 0  # ... and the last order_precedences call
        self.positions_fallback_rows = 0    # ... and the last order_positions call
        self.times_fallback_rows = 0        # ... and the last order_times call
        self.snapshots_fallback_rows = 0    # ... and the last order_snapshots call
        self.samples_fallback_rows = 0      # ... and the last sample_orders call

    # ------------------------------------------------------------------ diagonals
    def _get_diag_unpaired(self, state: State, seeding: bool = True) -> np.ndarray:
        """model.py:378-432."""
        nn = self.n + 1 if seeding else self.n
        return _single_diag(self.log_theta, nn, [j for j in range(nn) if j in state])

    def _get_diag_paired(self, state: MetState) -> np.ndarray:
        """model.py:434-446: on the device, through mmhn_kron_diag."""
        return np.asarray(_kronvec.kron_diag(self.log_theta, state.to_seq().astype(np.int32), len(state)),
                          dtype=np.float64)

    # ------------------------------------------------------------------ public entry points
    def _route(self, state, met_status: str, first_obs: str):
        """The checks of model.py:213-293: which chain a (state, status) pair runs on - "mt" / "pt" with its one-tumour
        state, "paired" with the MetState."""
        if isinstance(state, np.ndarray):
            state = MetState.from_seq(state)
        if met_status == "isMetastasis":
            if len(state.PT) > 0:
                raise ValueError("PT part of the state was not empty, but met_status is 'isMetastasis'.")
            if not state.Seeding:
                raise ValueError("Seeding was not observed, but met_status is 'isMetastasis'.")
            return "mt", state.MT
        if met_status == "absent":
            if len(state.MT) > 0 or state.MT_events:
                raise ValueError("Met part of the state was not empty, but met_status is 'absent'.")
            if state.Seeding:
                raise ValueError("Seeding was observed, but met_status is 'absent'.")
            return "pt", state.PT_S
        if met_status == "present":
            if tuple(state.MT) != (self.n,):
                raise ValueError("Met part of the state was not empty, but met_status is 'present', not 'isPaired'.")
            return "pt", state.PT_S
        if met_status == "isPaired":
            if first_obs not in _FIRST_OBS:
                raise ValueError(_FIRST_ERR)
            if first_obs == "sync":
                warnings.warn("Synchronous development is deprecated.", DeprecationWarning)
            return "paired", state
        raise ValueError(_STATUS_ERR)

    def likeliest_order(self, state, met_status: str, first_obs: str = None):
        """model.py:213-293: (order, probability)."""
        chain, st = self._route(state, met_status, first_obs)
        if chain == "mt":
            return self._likeliest_order_unpaired_mt(st)
        if chain == "pt":
            return self._likeliest_order_unpaired_pt(st)
        return self._likeliest_order_paired(st, first_obs)

    def likeliest_orders(self, dat, backend: str = "device", front_cap: int = 0) -> list:
        """The likeliest order of every row of a reference-format `dat` [n_pat, 2n+3]: a list of (order, probability),
        order a tuple of event codes, equal to likeliest_order row by row.  The type column dat[:, -1] gives the status
        (0 "absent", 1 "present", 2 "isMetastasis", 3 "isPaired"), the diagnosis order dat[:, -2] a paired row's first
        observation (0 "unknown", 1 "PT", 2 - or any other value, as the objective reads it - "Met").

        backend="device": every row in one call of the HIP library (mmhn_likeliest_orders); a row whose Pareto front
        outgrew `front_cap` candidates (0: the library's default) or whose lattice does not fit the workspace is
        recomputed here with likeliest_order - how many did is left in `self.orders_fallback_rows`.
        backend="host": likeliest_order row by row.  An invalid row raises likeliest_order's ValueError, with its index."""
        dat = np.asarray(dat)
        if dat.ndim != 2 or dat.shape[1] != 2 * self.n + 3:
            raise ValueError(f"dat must have shape [n_pat, {2 * self.n + 3}]")
        if backend == "host":
            self.orders_fallback_rows = 0
            return [self._row_order(dat, i) for i in range(dat.shape[0])]
        if backend != "device":
            raise ValueError("backend must be 'device' or 'host'")
        from .jx import engine
        orders, prob, status = engine(self.n).likeliest_orders(self.log_theta, self.obs1, self.obs2, dat, front_cap)
        bad = np.flatnonzero(status == 2)
        if bad.size:
            i = int(bad[0])
            raise ValueError(f"row {i}: {_ROW_ERRORS[int(orders[i, 0])]}")
        out, fallback = [], 0
        for i in range(dat.shape[0]):
            if status[i] == 0:
                out.append((tuple(int(e) for e in orders[i] if e >= 0), float(prob[i])))
            else:
                out.append(self._row_order(dat, i))
                fallback += 1
        self.orders_fallback_rows = fallback
        return out

    def _row_args(self, dat, i: int):
        """Row i of a reference-format dat as the (state, met_status, first_obs) of the one-observation entry points."""
        row = dat[i]
        status = _ROW_STATUS.get(int(row[-1]), f"type {int(row[-1])}")
        first = _ROW_FIRST.get(int(row[-2]), "Met") if status == "isPaired" else None
        return MetState.from_seq(row[:2 * self.n + 1]), status, first

    def _row_order(self, dat, i: int):
        try:
            order, p = self.likeliest_order(*self._row_args(dat, i))
        except ValueError as e:
            raise ValueError(f"row {i}: {e}") from e
        return tuple(int(e) for e in order), float(p)

    def _order_cohort(self, device, one, fields: tuple, shapes: tuple, dat, backend: str, dtypes: tuple = None,
                      with_row: bool = False) -> list:
        """What order_posteriors / order_precedences / order_positions / order_times / order_snapshots / sample_orders share: [log_evidence,
        the arrays of `fields` ..., the number of rows the device turned away] of every row of dat, from the Engine method
        `device(engine)` with the rows it turned away recomputed by `one` (the entry point of one observation), or from
        `one` alone (backend="host").  dtypes: of the arrays of `fields` (float64 each by default); with_row: `one` also
        takes the row's index (row=i)."""
        dat = np.asarray(dat)
        if dat.ndim != 2 or dat.shape[1] != 2 * self.n + 3:
            raise ValueError(f"dat must have shape [n_pat, {2 * self.n + 3}]")
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        P = dat.shape[0]
        if backend == "host":
            kinds = (np.float64,) + tuple(dtypes or (np.float64,) * len(shapes))
            out = [np.zeros((P,) + shape, dtype=kind) for shape, kind in zip(((),) + shapes, kinds)]
            redo = range(P)
        else:
            from .jx import engine
            *out, status = device(engine(self.n))(self.log_theta, self.obs1, self.obs2, dat)
            bad = np.flatnonzero((status & 0xFFFF) == 2)
            if bad.size:
                i = int(bad[0])
                raise ValueError(f"row {i}: {_ROW_ERRORS[int(status[i]) >> 16]}")
            redo = [int(i) for i in np.flatnonzero(status != 0)]
        for i in redo:
            try:
                r = one(*self._row_args(dat, i), row=i) if with_row else one(*self._row_args(dat, i))
            except ValueError as e:
                raise ValueError(f"row {i}: {e}") from e
            for a, field in zip(out, ("log_evidence",) + fields):
                a[i] = getattr(r, field)
        return out + [0 if backend == "host" else len(redo)]

    def order_posterior(self, state, met_status: str, first_obs: str = None) -> "OrderPosterior":
        """The sum over every admissible order where likeliest_order takes the maximum (same arguments, checks and
        errors): `log_evidence` = log of the summed order likelihoods, `pre[m]` = P(mutation m occurred before the seeding
        | the observation), `seed_pos[j]` = P(j mutations preceded the seeding | the observation).  Exact: a forward and a
        backward sum-product pass over the lattice of sub-states likeliest_order walks.  "absent" has no seeding to place:
        pre and seed_pos are NaN."""
        chain, st = self._route(state, met_status, first_obs)
        if chain == "mt":
            return self._posterior_single(self._single_tables(self.log_theta, st, self.obs2))
        if chain == "pt":
            return self._posterior_single(self._single_tables(self._pt_log_theta, st, self.obs1))
        return self._posterior_paired(st, first_obs)

    def order_posteriors(self, dat, backend: str = "device") -> "OrderPosteriors":
        """order_posterior of every row of a reference-format `dat` [n_pat, 2n+3], rows read as likeliest_orders reads
        them: arrays log_evidence [n_pat], pre [n_pat, n], seed_pos [n_pat, n+1].

        backend="device": every row in one call of the HIP library (mmhn_order_posteriors); a row whose lattice does not
        fit the workspace is recomputed here with order_posterior - how many were is left in
        `self.posteriors_fallback_rows`.  backend="host": order_posterior row by row.  An invalid row raises
        likeliest_order's ValueError, with its index."""
        shapes = ((self.n,), (self.n + 1,))
        *out, self.posteriors_fallback_rows = self._order_cohort(
            lambda eng: eng.order_posteriors, self.order_posterior, ("pre", "seed_pos"), shapes, dat, backend)
        return OrderPosteriors(*out)

    def order_precedence(self, state, met_status: str, first_obs: str = None) -> "OrderPrecedence":
        """Which of two events came first, summed over every admissible order (same arguments, checks and errors as
        order_posterior): `prec[c, d]` = P(code c happened strictly earlier than code d | the observation) over the event
        codes of likeliest_order (2i PT, 2i+1 MT, 2n seeding).  The two codes of an event that occurred before the
        seeding happen at the same moment: neither precedes the other.  Entries of codes the observation does not carry
        are NaN, the diagonal of those it carries is 0.  Exact: every order is a path of moves x -> y over the lattice
        likeliest_order walks, a move has the mass B[y] . A(x, b) F[x] (forward prefix vector, backward weight), and
        prec[c, d] is the summed mass of the moves that add d from a state that holds c, over the evidence."""
        chain, st = self._route(state, met_status, first_obs)
        if chain == "mt":
            T = self._single_tables(self.log_theta, st, self.obs2)
            return self._precedence_single(T, [2 * self.n if e == self.n else 2 * e + 1 for e in T.ev])
        if chain == "pt":
            T = self._single_tables(self._pt_log_theta, st, self.obs1)
            return self._precedence_single(T, [2 * e for e in T.ev])
        return self._precedence_paired(st, first_obs)

    def order_precedences(self, dat, backend: str = "device") -> "OrderPrecedences":
        """order_precedence of every row of a reference-format `dat` [n_pat, 2n+3], rows read as order_posteriors reads
        them: arrays log_evidence [n_pat], prec [n_pat, 2n+1, 2n+1].

        backend="device": every row in one call of the HIP library (mmhn_order_precedences); a row whose lattice does not
        fit the workspace is recomputed here with order_precedence - how many were is left in
        `self.precedences_fallback_rows`.  backend="host": order_precedence row by row.  An invalid row raises
        likeliest_order's ValueError, with its index."""
        L = 2 * self.n + 1
        *out, self.precedences_fallback_rows = self._order_cohort(
            lambda eng: eng.order_precedences, self.order_precedence, ("prec",), ((L, L),), dat, backend)
        return OrderPrecedences(*out)

    def order_position(self, state, met_status: str, first_obs: str = None) -> "OrderPosition":
        """At which position of its lineage every event happened, summed over every admissible order (same arguments,
        checks and errors as order_precedence): `pos_mt[e, j]` = P(event e - n: the seeding - is the j-th (0-based) entry of
        the MT lineage | the observation), `pos_pt` the same for the PT lineage.  The MT lineage of an order is the order
        without its even codes other than the seeding (the events before the seeding, the seeding, the metastasis' own
        events), the PT lineage the order without its odd codes.  "isMetastasis" has the MT lineage only, "present" and
        "absent" the PT lineage ("absent" without the seeding).  Rows of events the observation does not carry in a lineage
        are NaN, a lineage it does not have is NaN throughout; positions past the lineage's length are 0.  Exact: the move
        that adds slot d from the state x (mass as in order_precedence) puts d's event at the position
        popcount(x & the slots of d's lineage)."""
        chain, st = self._route(state, met_status, first_obs)
        nan = np.full((self.n + 1, self.n + 1), np.nan)
        if chain == "mt":
            le, pos = self._position_single(self._single_tables(self.log_theta, st, self.obs2))
            return OrderPosition(le, nan, pos)
        if chain == "pt":
            le, pos = self._position_single(self._single_tables(self._pt_log_theta, st, self.obs1))
            return OrderPosition(le, pos, nan)
        return self._position_paired(st, first_obs)

    def order_positions(self, dat, backend: str = "device") -> "OrderPositions":
        """order_position of every row of a reference-format `dat` [n_pat, 2n+3], rows read as order_posteriors reads
        them: arrays log_evidence [n_pat], pos_pt and pos_mt [n_pat, n+1, n+1].

        backend="device": every row in one call of the HIP library (mmhn_order_positions); a row whose lattice does not
        fit the workspace is recomputed here with order_position - how many were is left in
        `self.positions_fallback_rows`.  backend="host": order_position row by row.  An invalid row raises
        likeliest_order's ValueError, with its index."""
        NN = (self.n + 1, self.n + 1)
        *out, self.positions_fallback_rows = self._order_cohort(
            lambda eng: eng.order_positions, self.order_position, ("pos_pt", "pos_mt"), (NN, NN), dat, backend)
        return OrderPositions(*out)

    def order_time(self, state, met_status: str, first_obs: str = None) -> "OrderTime":
        """When every event and every observation happened, summed over every admissible order and every point of it at
        which the first observation can fall (same arguments, checks and errors as order_precedence): `time[c]` = the
        posterior mean of the time of the event with code c (2i PT, 2i+1 MT, 2n seeding; NaN where the observation does
        not carry it), `obs` = the posterior mean times of the first and the second observation (one tumour: its
        observation, NaN), `pt_first` = P(the primary tumour was observed first | the observation) - exactly 1.0 for
        first_obs "PT", 0.0 for "Met", NaN for "sync" and for one tumour.  Time 0 is the event-free state; an event-free
        tumour is observed at rate 1.  Exact: given a path the chain holds in a state x for an Exp(den[x]) time that does
        not depend on the move that follows, so a mean time is the sum over the lattice of (the probability that the chain
        passes through x in a regime, forward vector times backward weight over the evidence) / (that regime's den[x]) over
        the states before the moment in question - for the event of a slot, the states that do not hold the slot."""
        chain, st = self._route(state, met_status, first_obs)
        if chain == "mt":
            T = self._single_tables(self.log_theta, st, self.obs2)
            return self._time_single(T, [2 * self.n if e == self.n else 2 * e + 1 for e in T.ev])
        if chain == "pt":
            T = self._single_tables(self._pt_log_theta, st, self.obs1)
            return self._time_single(T, [2 * e for e in T.ev])
        return self._time_paired(st, first_obs)

    def order_times(self, dat, backend: str = "device") -> "OrderTimes":
        """order_time of every row of a reference-format `dat` [n_pat, 2n+3], rows read as order_posteriors reads them:
        arrays log_evidence [n_pat], time [n_pat, 2n+1], obs [n_pat, 2], pt_first [n_pat].

        backend="device": every row in one call of the HIP library (mmhn_order_times); a row whose lattice does not fit the
        workspace is recomputed here with order_time - how many were is left in `self.times_fallback_rows`.
        backend="host": order_time row by row.  An invalid row raises likeliest_order's ValueError, with its index."""
        shapes = ((2 * self.n + 1,), (2,), ())
        *out, self.times_fallback_rows = self._order_cohort(
            lambda eng: eng.order_times, self.order_time, ("time", "obs", "pt_first"), shapes, dat, backend)
        return OrderTimes(*out)

    def order_snapshot(self, state, met_status: str, first_obs: str = None) -> "OrderSnapshot":
        """What the two tumours looked like at the moment of the first observation, summed over every admissible order and
        every point of it at which the first observation can fall (same arguments, checks and errors as order_precedence).
        With r = 0 the primary tumour observed first and r = 1 the metastasis: `held[r, c]` = P(the first observation was of
        tumour r and the event with code c - 2i PT, 2i+1 MT, 2n seeding - had happened by then | the observation), so
        held[0, 2n] + held[1, 2n] = 1, held[0, 2n] is order_time's pt_first and held[r, c] = held[r, 2n] for the codes of
        tumour r itself; `late[r, j]` = P(the first observation was of tumour r and exactly j events of the other tumour
        happened after it | the observation), 0 past the number of events the other tumour has, the whole block summing to
        1; `map_first`, `map_state`, `map_prob`: the single most probable (r, state at the first observation) - of equal
        masses r = 0 before r = 1, then the state that is the smaller number over the observation's slots - and its
        probability.  Exact: the first observation falls in a seeded state x that holds every event of the tumour it is made
        of, and with _paired_passes' F, B and Z the mass F[x]_a o1[x] / den_mt[x] B[x]_P (the primary tumour; F[x]_a o2[x] /
        den_pt[x] B[x]_M the metastasis) over Z is the posterior probability that it fell there.  One tumour has one
        observation and "sync" no first one: log_evidence, NaN and -1 elsewhere."""
        chain, st = self._route(state, met_status, first_obs)
        if chain == "mt":
            Z = self._single_passes(self._single_tables(self.log_theta, st, self.obs2))[1]
            return self._snapshot_none(float(np.log(Z)))
        if chain == "pt":
            Z = self._single_passes(self._single_tables(self._pt_log_theta, st, self.obs1))[1]
            return self._snapshot_none(float(np.log(Z)))
        return self._snapshot_paired(st, first_obs)

    def order_snapshots(self, dat, backend: str = "device") -> "OrderSnapshots":
        """order_snapshot of every row of a reference-format `dat` [n_pat, 2n+3], rows read as order_posteriors reads them:
        arrays log_evidence [n_pat], held [n_pat, 2, 2n+1], late [n_pat, 2, n+1], map_state [n_pat, 2n+1] (int8), map_first
        [n_pat] (int32), map_prob [n_pat].

        backend="device": every row in one call of the HIP library (mmhn_order_snapshots); a row whose lattice does not fit
        the workspace is recomputed here with order_snapshot - how many were is left in `self.snapshots_fallback_rows`.
        backend="host": order_snapshot row by row.  An invalid row raises likeliest_order's ValueError, with its index."""
        L = 2 * self.n + 1
        *out, self.snapshots_fallback_rows = self._order_cohort(
            lambda eng: eng.order_snapshots, self.order_snapshot, ("held", "late", "map_state", "map_first", "map_prob"),
            ((2, L), (2, self.n + 1), (L,), (), ()), dat, backend,
            dtypes=(np.float64, np.float64, np.int8, np.int32, np.float64))
        return OrderSnapshots(*out)

    def sample_order(self, state, met_status: str, first_obs: str = None, n_samples: int = 1, key: int = 0, first: int = 0,
                     row: int = 0) -> "OrderSample":
        """Orders drawn from the exact posterior over the admissible orders of one observation (same arguments, checks and
        errors as order_posterior): an order comes with the probability likelihood(order) / evidence.  This is the
        definition the device kernel (csrc/ordersample.h: k_order_sample) follows operation by operation.

        A path starts at the empty sub-state and makes moves up to the full state.  The candidates of a move are visited
        in a fixed order, their weights w - the move's factor times the backward weight of the state it leads to - summed
        in that order to `total`; the move taken is the first candidate whose cumulative weight exceeds u * total (if
        rounding lets the loop fall through, the last candidate with w > 0: gillespie_step's rule), and log_prob
        accumulates log(w / total).
          one tumour              from x every slot b not in x, ascending: w = num_b[x | b] G[x | b]  (_single_passes)
          paired, before seeding  from the joint events e the joint move of every event not in e, ascending (its PT code,
                                  then its MT code), then the seeding: _unseeded_backward's terms, total = Bu
          paired, after seeding   the path carries its own prefix vector f; at x, (fa, fp, fm) = _settle(x, f), every slot
                                  b < k - 1 not in x, ascending, y = x | b: g = _advance's vector, w = B[y] . g, and
                                  f = g / w after the choice, so that the next total is 1 up to rounding.  The seeding move
                                  is a choice like any other: it leaves f = (1 / B[y]_a, 0, 0)
        u: one Philox4x32-10 uniform per move (_philox.order_uniforms), key = the 64-bit `key`, counter = (sample index low
        word, high word, move number, row + 1) for the sample indices first ... first + n_samples - 1: a sample depends on
        (key, row, its index) only."""
        n_samples, first = int(n_samples), int(first)
        if n_samples < 0 or first < 0:
            raise ValueError(f"n_samples and first must be non-negative, got n_samples={n_samples}, first={first}")
        chain, st = self._route(state, met_status, first_obs)
        samples = np.uint64(first) + np.arange(n_samples, dtype=np.uint64)
        if chain == "mt":
            T = self._single_tables(self.log_theta, st, self.obs2)
            return self._sample_single(T, [2 * self.n if e == self.n else 2 * e + 1 for e in T.ev], samples, key, row)
        if chain == "pt":
            T = self._single_tables(self._pt_log_theta, st, self.obs1)
            return self._sample_single(T, [2 * e for e in T.ev], samples, key, row)
        return self._sample_paired(st, first_obs, samples, key, row)

    def sample_orders(self, dat, n_samples: int, key: int = 0, first: int = 0, backend: str = "device") -> "OrderSamples":
        """sample_order of every row of a reference-format `dat` [n_pat, 2n+3], rows read as order_posteriors reads them,
        row i with row=i: arrays log_evidence [n_pat], orders [n_pat, n_samples, 2n+1] (int8), log_prob [n_pat, n_samples].

        backend="device": every row in one call of the HIP library (mmhn_order_samples); a row whose lattice and samples
        do not fit the workspace is drawn here with sample_order - how many were is left in `self.samples_fallback_rows`.
        backend="host": sample_order row by row.  An invalid row raises likeliest_order's ValueError, with its index."""
        dat = np.asarray(dat)
        if dat.ndim != 2 or dat.shape[1] != 2 * self.n + 3:
            raise ValueError(f"dat must have shape [n_pat, {2 * self.n + 3}]")
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        n_samples, first = int(n_samples), int(first)
        if n_samples < 0 or first < 0:
            raise ValueError(f"n_samples and first must be non-negative, got n_samples={n_samples}, first={first}")
        *out, self.samples_fallback_rows = self._order_cohort(
            lambda eng: lambda lt, o1, o2, d: eng.order_samples(lt, o1, o2, d, n_samples, key, first),
            lambda st, status, fo, row: self.sample_order(st, status, fo, n_samples, key, first, row),
            ("orders", "log_prob"), ((n_samples, 2 * self.n + 1), (n_samples,)), dat, backend,
            dtypes=(np.int8, np.float64), with_row=True)
        return OrderSamples(*out)

    # ------------------------------------------------------------------ seeding forecasts
    def _forecast_checks(self, genotypes, until: str) -> np.ndarray:
        """The genotypes as an int array [R, n]; the errors of seeding_forecast / seeding_forecasts."""
        if until not in _FORECAST_UNTIL:
            raise ValueError("until must be 'seeding' or 'observation'")
        g = np.asarray(genotypes)
        if g.ndim != 2 or g.shape[1] != self.n:
            raise ValueError(f"genotypes must have shape [R, {self.n}]")
        bad = np.flatnonzero(~np.isin(g, (0, 1)).all(axis=1))
        if bad.size:
            raise ValueError(f"row {int(bad[0])}: a genotype entry is neither 0 nor 1")
        th = self._pt_log_theta
        if until == "seeding" and np.exp(th[self.n, self.n] + th[self.n, :self.n].sum()) == 0.0:
            raise ValueError(_NO_SEEDING_EXIT)
        return g.astype(np.int64)

    def _forecast_next(self, g: np.ndarray, until: str) -> np.ndarray:
        """next [R, n+1] of the genotypes g [R, n]: the rates out of the genotype over their sum with the clock."""
        th, n = self._pt_log_theta, self.n
        rate = np.exp(np.diag(th)[None, :] + g @ th[:, :n].T)                      # [R, n+1]: lambda_j(x), sigma(x)
        rate[:, :n] = np.where(g == 1, 0.0, rate[:, :n])
        kap = np.exp(g @ self.obs1[:n]) if until == "observation" else 0.0
        out = rate / (rate.sum(axis=1) + kap)[:, None]
        out[:, :n] = np.where(g == 1, np.nan, out[:, :n])
        return out

    def seeding_forecast(self, genotype, until: str = "seeding") -> "SeedingForecast":
        """The forward question: a primary tumour holds the mutations of `genotype` (n entries 0 / 1) and has not seeded -
        what happens until the seeding (until="seeding"), or until the seeding or the first observation on the model's own
        clock, whichever comes first (until="observation")?  See SeedingForecast for the answers.

        Exact: before the seeding the chain runs on the supersets y of the genotype, a lattice over the f mutations it does
        not hold, with rates lambda_j(y) = exp(theta_jj + sum_{i in y} theta_ji) (j not in y), sigma(y) the same for the
        seeding (the primary tumour's theta: theta[:n, n] is not read) and kappa(y) = exp(sum_{i in y} obs1_i) for the clock
        (0 until the seeding); den = sum lambda + sigma + kappa.  F(genotype) = 1, F(y) = sum_b F(y - b) lambda_b(y - b) /
        den(y - b) is the probability of reaching y, G = F / den the expected time spent there, and every answer is a sum of
        G times a rate.  This is the host definition, level by level in NumPy (f <= 24); seeding_forecasts has the device."""
        g = self._forecast_checks(np.asarray(genotype)[None, :] if np.ndim(genotype) == 1 else genotype, until)
        if g.shape[0] != 1:
            raise ValueError("seeding_forecast takes one genotype; seeding_forecasts takes many")
        g = g[0]
        th, n = self._pt_log_theta, self.n
        held = [i for i in range(n) if g[i]]
        free = [i for i in range(n) if not g[i]]
        f = len(free)
        if f > _FORECAST_HOST_MAX:
            raise ValueError(f"{f} free mutations: the host definition stops at {_FORECAST_HOST_MAX} "
                             f"(a lattice of 2^{f} states x {f} rates); use seeding_forecasts, backend='device'")
        idx = np.arange(1 << f)
        level = _subset_sums(np.ones(f)).astype(np.int64)
        # rate of j in the state y (its own bit does not count: rows of j-free states are the only ones read)
        lam = [np.exp(th[j, j] + th[j, held].sum() + _subset_sums(th[j, free])) for j in free]
        sig = np.exp(th[n, n] + th[n, held].sum() + _subset_sums(th[n, free]))
        kap = np.exp(self.obs1[held].sum() + _subset_sums(self.obs1[free])) if until == "observation" else np.zeros(1 << f)
        out = [(idx >> a & 1) == 0 for a in range(f)]
        den = np.zeros(1 << f)
        for a in range(f):
            den += np.where(out[a], lam[a], 0.0)
        den = den + sig + kap
        F, G = np.zeros(1 << f), np.zeros(1 << f)
        F[0] = 1.0
        for lev in range(f + 1):
            ys = idx[level == lev]
            for a in range(f if lev else 0):
                to = ys[(ys >> a & 1) == 1]
                frm = to ^ (1 << a)
                F[to] += G[frm] * lam[a][frm]
            G[ys] = F[ys] / den[ys]
        gs = G * sig
        before, with_seed = np.full(n, np.nan), np.full(n, np.nan)
        for a, j in enumerate(free):
            before[j] = float((G * lam[a])[out[a]].sum())
            with_seed[j] = float(gs[~out[a]].sum())
        n_before = np.zeros(n + 1)
        for m in range(f + 1):
            n_before[m] = float(gs[level == m].sum())
        return SeedingForecast(float(gs.sum()), float(G.sum()), before, with_seed, n_before,
                               self._forecast_next(g[None, :], until)[0])

    def seeding_forecasts(self, genotypes, until: str = "seeding", backend: str = "device") -> "SeedingForecasts":
        """seeding_forecast of every row of `genotypes` [R, n] (of a cohort `dat`: dat[:, 0:2*n:2], the primary tumours'
        columns): arrays p_seed [R], time [R], before [R, n], with_seed [R, n], n_before [R, n+1], next [R, n+1].
        Identical genotypes are solved once.

        backend="device": every distinct genotype in one call of the HIP library (mmhn_seeding_forecasts), a lattice of
        8 B x 2^f per row spread over the whole GPU, level by level.  A row that does not fit (more than 30 free mutations,
        or a lattice larger than the workspace limit) raises a ValueError that names the row and the bytes it needs: there
        is no host fallback, a host lattice of 2^28 states is none.  backend="host": seeding_forecast row by row.
        An entry other than 0 / 1 raises ValueError("row i: ...")."""
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        g = self._forecast_checks(genotypes, until)
        R, n = g.shape[0], self.n
        uniq, first, inverse = np.unique(g, axis=0, return_index=True, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        if backend == "host":
            rows = [self.seeding_forecast(u, until) for u in uniq]
            cols = [np.array([getattr(r, name) for r in rows], dtype=np.float64).reshape((len(rows),) + shape)
                    for name, shape in (("p_seed", ()), ("time", ()), ("before", (n,)), ("with_seed", (n,)),
                                        ("n_before", (n + 1,)))]
        else:
            from .jx import engine
            *cols, status = engine(n).seeding_forecasts(self.log_theta, self.obs1, uniq.astype(np.int8), until)
            bad = np.flatnonzero(status != 0)
            if bad.size:
                u = int(bad[0])
                i, f = int(first[u]), int(n - uniq[u].sum())
                if (int(status[u]) & 0xFFFF) == 2:
                    raise ValueError(f"row {i}: a genotype entry is neither 0 nor 1")
                raise ValueError(f"row {i}: {f} free mutations, a lattice of 2^{f} states that needs {8 << f} bytes "
                                 "(at most 30 free mutations, and the lattice has to fit the workspace limit); "
                                 "there is no host fallback")
        return SeedingForecasts(*(c[inverse] for c in cols), self._forecast_next(g, until))

    # ------------------------------------------------------------------ sweeps over all 2^n genotypes: what the three share
    def _lattice_host_rates(self, what: str):
        """idx, level (the popcount), lam [n] and sig over the 2^n genotype codes for the host definition of the `what`."""
        th, n = self._pt_log_theta, self.n
        if n > _LATTICE_HOST_MAX:
            raise ValueError(f"{n} mutations: the host {what} stops at {_LATTICE_HOST_MAX} ({n} x 2^{n} doubles of "
                             "rates); use backend='device'")
        idx = np.arange(1 << n)
        level = _subset_sums(np.ones(n)).astype(np.int64)
        lam = [np.exp(th[j, j] + _subset_sums(np.where(np.arange(n) == j, 0.0, th[j, :n]))) for j in range(n)]
        sig = np.exp(th[n, n] + _subset_sums(th[n, :n]))
        return idx, level, lam, sig

    def _lattice_whole(self, backend, max_bytes, planes, noun, prep, at, host, device, result, summary_host=None, summary=None):
        """The body of seeding_landscape, genotype_distribution and metastasis_distribution behind their own checks: every
        genotype's `planes` values, from host() [planes, 2^n] (with summary_host of it) or from device(engine, genotypes,
        full) -> values, status, sums, whole (with summary(*sums)).  `noun`, `prep` and `at` word the refusal of max_bytes."""
        n = self.n
        if backend == "host" and n > _LATTICE_HOST_MAX:
            host()                                  # (raises: the message points to the device)
        self._lattice_max_bytes(max_bytes, planes, noun, prep, at)
        if backend == "host":
            whole = host()
            sums = summary_host(whole) if summary_host else None
        else:
            from .jx import engine
            _, _, sums, whole = device(engine(n), np.zeros((0, n), dtype=np.int8), True)
            sums = summary(*sums) if summary else None
        return result(*whole, np.arange(1 << n), *(() if sums is None else (sums,)))

    def _lattice_at(self, genotypes, until, backend, planes, host, device, result, summary_host=None, summary=None):
        """The body of the three _at methods behind the backend check: _lattice_whole's values at the rows of `genotypes`."""
        g = self._forecast_checks(genotypes, until)
        n = self.n
        codes = g @ (1 << np.arange(n, dtype=np.int64))
        if backend == "host":
            whole = host()
            values, sums = whole[:, codes].T, summary_host(whole) if summary_host else None
        else:
            from .jx import engine
            values, status, sums, _ = device(engine(n), g.astype(np.int8), False)
            bad = np.flatnonzero(status != 0)
            if bad.size:
                raise ValueError(f"row {int(bad[0])}: a genotype entry is neither 0 nor 1")
            sums = summary(*sums) if summary else None
        return result(*(np.ascontiguousarray(values[:, k]) for k in range(planes)), codes, *(() if sums is None else (sums,)))

    # ------------------------------------------------------------------ seeding landscape
    def _landscape_host(self, until: str) -> np.ndarray:
        """[4, 2^n]: the definition of the landscape, level by level over the popcount of the code, descending."""
        n, size = self.n, 1 << self.n
        idx, level, lam, sig = self._lattice_host_rates("landscape")
        kap = np.exp(_subset_sums(self.obs1[:n])) if until == "observation" else np.zeros(size)
        p, t, e, s = (np.zeros(size) for _ in range(4))
        for lev in range(n, -1, -1):
            xs = idx[level == lev]
            n0, n1, n2, n3, den = (np.zeros(len(xs)) for _ in range(5))
            for j in range(n):
                m = (xs >> j & 1) == 0
                x = xs[m]
                y = x | 1 << j
                r = lam[j][x]
                n0[m] += r * p[y]
                n1[m] += r * t[y]
                n2[m] += r * (1.0 + e[y])
                n3[m] += r * (p[y] + s[y])
                den[m] += r
            den = den + sig[xs] + kap[xs]
            p[xs] = (sig[xs] + n0) / den
            t[xs] = (1.0 + n1) / den
            e[xs] = n2 / den
            s[xs] = n3 / den
        return np.stack((p, t, e, s))

    def seeding_landscape(self, until: str = "seeding", backend: str = "device", max_bytes: int = 2 ** 31) -> "SeedingLandscape":
        """seeding_forecast's p_seed, time, sum of before and sum of with_seed of EVERY genotype of the model: arrays over
        the 2^n genotype codes (bit j of a code = mutation j held), from one backward pass over the lattice of all genotypes
        instead of a forward pass per genotype.  With the rates of seeding_forecast and j over the mutations x does not hold:
            p_seed(x)      = (sigma(x) + sum_j lambda_j(x) p_seed(x + j)) / den(x)
            time(x)        = (1 + sum_j lambda_j(x) time(x + j)) / den(x)
            new_events(x)  = sum_j lambda_j(x) (1 + new_events(x + j)) / den(x)
            seed_events(x) = sum_j lambda_j(x) (p_seed(x + j) + seed_events(x + j)) / den(x)
        starting at the full genotype, which has no j.

        backend="device": one call of the HIP library (mmhn_seeding_landscape), 32 B x 2^n of workspace and as much here for
        the result; a ValueError names the bytes when that exceeds `max_bytes` (2 GiB: n <= 26).  backend="host": the
        definition in NumPy, level by level, n <= 24."""
        if until not in _FORECAST_UNTIL:
            raise ValueError("until must be 'seeding' or 'observation'")
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        th, n = self._pt_log_theta, self.n
        if until == "seeding" and np.exp(th[n, n] + th[n, :n].sum()) == 0.0:
            raise ValueError(_NO_SEEDING_EXIT)
        return self._lattice_whole(backend, max_bytes, 4, "landscape", "of", "seeding_landscape_at",
                                   lambda: self._landscape_host(until), self._landscape_device(until), SeedingLandscape)

    def _landscape_device(self, until: str):
        def device(eng, g, full):
            values, status, whole = eng.seeding_landscape(self.log_theta, self.obs1, g, until, full=full)
            return values, status, None, whole
        return device

    def seeding_landscape_at(self, genotypes, until: str = "seeding", backend: str = "device") -> "SeedingLandscape":
        """The four values of seeding_landscape at the rows of `genotypes` [R, n] (0 / 1), [R] each, with the rows' codes:
        the whole landscape is swept on the device (32 B x 2^n of its workspace, any n the engine takes) and only the rows
        come back - what a cohort of many rows needs, whatever its size.  backend="host": the NumPy landscape, n <= 24.
        An entry other than 0 / 1 raises ValueError("row i: ...") as seeding_forecasts does."""
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        return self._lattice_at(genotypes, until, backend, 4, lambda: self._landscape_host(until),
                                self._landscape_device(until), SeedingLandscape)

    # ------------------------------------------------------------------ genotype distribution of the primary tumour
    def _genodist_host(self) -> np.ndarray:
        """[2, 2^n]: the definition of the genotype distribution (U, S), level by level over the popcount, ascending."""
        n, size = self.n, 1 << self.n
        idx, level, lam, sig = self._lattice_host_rates("distribution")
        kap0 = np.exp(_subset_sums(self.obs1[:n]))
        kap1 = kap0 * np.exp(self.obs1[n])
        L = np.zeros(size)
        for j in range(n):
            L += np.where((idx >> j & 1) == 0, lam[j], 0.0)
        den0, den1 = L + sig + kap0, L + kap1
        F0, F1, G0, G1 = (np.zeros(size) for _ in range(4))
        F0[0] = 1.0
        for lev in range(n + 1):
            ys = idx[level == lev]
            for b in range(n if lev else 0):
                to = ys[(ys >> b & 1) == 1]
                frm = to ^ (1 << b)
                r = lam[b][frm]
                F0[to] += G0[frm] * r
                F1[to] += G1[frm] * r
            G0[ys] = F0[ys] / den0[ys]
            F1[ys] = G0[ys] * sig[ys] + F1[ys]
            G1[ys] = F1[ys] / den1[ys]
        return np.stack((kap0 * G0, kap1 * G1))

    @staticmethod
    def _genodist_summary_host(P: np.ndarray) -> "GenotypeSummary":
        """The GenotypeSummary of the two planes P [2, 2^n], by its definition."""
        n = P.shape[1].bit_length() - 1
        level = _subset_sums(np.ones(n)).astype(np.int64)
        pairs, burden = np.zeros((2, n, n)), np.zeros((2, n + 1))
        for s in range(2):
            burden[s] = np.bincount(level, weights=P[s], minlength=n + 1)
            cube = P[s].reshape((2,) * n)                    # axis n - 1 - j is bit j
            for j in range(n):
                held = cube.take(1, axis=n - 1 - j)          # (bit i < j is axis n - 2 - i of what remains)
                pairs[s, j, j] = held.sum()
                for i in range(j):
                    pairs[s, i, j] = pairs[s, j, i] = held.take(1, axis=n - 2 - i).sum()
        return GenotypeSummary(P.sum(axis=1), pairs, burden)

    def genotype_distribution(self, backend: str = "device", max_bytes: int = 2 ** 31) -> "GenotypeDistribution":
        """The model's distribution over ALL genotypes of the primary tumour at its observation, split by whether the
        seeding has happened by then: arrays over the 2^n genotype codes (bit j of a code = mutation j held), from one forward
        pass over the lattice of all genotypes.  The primary tumour is an autonomous chain on (genotype, seeded or not) -
        theta[:n, n] is not read, the metastasis never acts on it.  With lambda_j(x) = exp(theta_jj + sum_{i in x}
        theta_ji), sigma(x) the same for the seeding, kappa0(x) = exp(sum_{i in x} obs1_i), kappa1 = kappa0 exp(obs1_n),
        L(x) the sum of lambda_j over the mutations x does not hold, b over the ones it holds:
            F0(empty) = 1,  F0(y) = sum_b G0(y - b) lambda_b(y - b),                    G0 = F0 / (L + sigma + kappa0)
                            F1(y) = G0(y) sigma(y) + sum_b G1(y - b) lambda_b(y - b),   G1 = F1 / (L + kappa1)
            unseeded = kappa0 G0 (exp(lp) of the type-0 row),  seeded = kappa1 G1 (exp(lp) of the type-1 row)
        `total` is the type-4 likelihood and sums to 1 over the genotypes, `p_seeded` is met_status_posterior's value and
        `summary` the exact marginal and pairwise frequencies and burden distributions of both planes (GenotypeSummary).  The
        reference's sibling package calls the one-plane form generate_pTh.

        backend="device": one call of the HIP library (mmhn_genotype_distribution), 16 B x 2^n of workspace and as much here
        for the result; a ValueError names the bytes when that exceeds `max_bytes` (2 GiB: n <= 27).  backend="host": the
        definition in NumPy, level by level, n <= 24."""
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        return self._lattice_whole(backend, max_bytes, 2, "distribution", "over", "genotype_distribution_at",
                                   self._genodist_host, self._genodist_device, GenotypeDistribution,
                                   self._genodist_summary_host, GenotypeSummary)

    def _genodist_device(self, eng, g, full):
        return eng.genotype_distribution(self.log_theta, self.obs1, g, summary=True, full=full)

    def genotype_distribution_at(self, genotypes, backend: str = "device") -> "GenotypeDistribution":
        """genotype_distribution's two values at the rows of `genotypes` [R, n] (0 / 1), [R] each, with the rows' codes and
        the summary of the WHOLE lattice: the distribution is swept on the device (16 B x 2^n of its workspace, any n the
        engine takes) and only the rows and the summary come back.  backend="host": the NumPy definition, n <= 24.
        An entry other than 0 / 1 raises ValueError("row i: ...") as seeding_forecasts does."""
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        return self._lattice_at(genotypes, "observation", backend, 2, self._genodist_host, self._genodist_device,
                                GenotypeDistribution, self._genodist_summary_host, GenotypeSummary)

    # ------------------------------------------------------------------ genotype distribution of the metastasis and its founder
    def _metdist_host(self) -> np.ndarray:
        """[3, 2^n]: the definition of the metastasis distribution (Z, M, C), level by level over the popcount, ascending."""
        n, size = self.n, 1 << self.n
        idx, level, lam, sig = self._lattice_host_rates("distribution")
        mu = [lam[j] * np.exp(self.log_theta[j, n]) for j in range(n)]
        kap0 = np.exp(_subset_sums(self.obs1[:n]))
        kapm = np.exp(self.obs2[n] + _subset_sums(self.obs2[:n]))
        L, Lm = np.zeros(size), np.zeros(size)
        for j in range(n):
            free = (idx >> j & 1) == 0
            L += np.where(free, lam[j], 0.0)
            Lm += np.where(free, mu[j], 0.0)
        den0, denm = L + sig + kap0, Lm + kapm
        F0, FM, FC, G0, GM, GC = (np.zeros(size) for _ in range(6))
        F0[0] = 1.0
        for lev in range(n + 1):
            ys = idx[level == lev]
            for b in range(n if lev else 0):
                to = ys[(ys >> b & 1) == 1]
                frm = to ^ (1 << b)
                F0[to] += G0[frm] * lam[b][frm]
                FM[to] += GM[frm] * mu[b][frm]
                FC[to] += GC[frm] * mu[b][frm]
            G0[ys] = F0[ys] / den0[ys]
            seeded = G0[ys] * sig[ys]
            FM[ys] = seeded + FM[ys]
            FC[ys] = seeded * lev + FC[ys]
            GM[ys] = FM[ys] / denm[ys]
            GC[ys] = FC[ys] / denm[ys]
        return np.stack((sig * G0, kapm * GM, kapm * GC))

    @staticmethod
    def _metdist_summary_host(P: np.ndarray) -> "MetastasisSummary":
        """The MetastasisSummary of the planes P [3, 2^n] (Z and M are summed), by its definition."""
        s = MetMHN._genodist_summary_host(P[:2])
        return MetastasisSummary(s.mass, s.pairs, s.burden)

    def metastasis_distribution(self, backend: str = "device", max_bytes: int = 2 ** 31) -> "MetastasisDistribution":
        """The model's distribution over ALL genotypes of the metastasis at its observation and of its founder, the cell
        that seeds: arrays over the 2^n genotype codes (bit j of a code = mutation j held), from one forward pass over the
        lattice of all genotypes.  The metastasis is an autonomous chain: the common lineage until the seeding (which the
        primary tumour's first observation can forestall), then its own rates, which carry the seeding's effect
        theta[:n, n], until its own clock obs2.  With genotype_distribution's lambda, sigma, kappa0, L and
        mu_j(z) = lambda_j(z) exp(theta_jn), Lm(z) the sum of mu_j over the mutations z does not hold,
        kappam(z) = exp(obs2_n + sum_{i in z} obs2_i), b over the mutations a genotype holds:
            F0(empty) = 1,  F0(y) = sum_b G0(y - b) lambda_b(y - b),                     G0 = F0 / (L + sigma + kappa0)
                            FM(y) = G0(y) sigma(y)     + sum_b GM(y - b) mu_b(y - b),    GM = FM / (Lm + kappam)
                            FC(y) = G0(y) sigma(y) |y| + sum_b GC(y - b) mu_b(y - b),    GC = FC / (Lm + kappam)
            founder = sigma G0,  metastasis = kappam GM (exp(lp) of the type-2 row),  founder_weighted = kappam GC
        `founder` and `metastasis` both sum to genotype_distribution's mass[1]; `founder_events` = founder_weighted /
        metastasis is the expected number of the metastasis' mutations that were already in the founder; `summary` holds the
        exact marginal and pairwise frequencies and burden distributions of the founder and the metastasis
        (MetastasisSummary).

        backend="device": one call of the HIP library (mmhn_metastasis_distribution), 24 B x 2^n of workspace and as much
        here for the result; a ValueError names the bytes when that exceeds `max_bytes` (2 GiB: n <= 26).  backend="host": the
        definition in NumPy, level by level, n <= 24."""
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        return self._lattice_whole(backend, max_bytes, 3, "distribution", "over", "metastasis_distribution_at",
                                   self._metdist_host, self._metdist_device, MetastasisDistribution,
                                   self._metdist_summary_host, MetastasisSummary)

    def _metdist_device(self, eng, g, full):
        return eng.metastasis_distribution(self.log_theta, self.obs1, self.obs2, g, summary=True, full=full)

    def metastasis_distribution_at(self, genotypes, backend: str = "device") -> "MetastasisDistribution":
        """metastasis_distribution's three values at the rows of `genotypes` [R, n] (0 / 1), [R] each, with the rows' codes
        and the summary of the WHOLE lattice: the distribution is swept on the device (24 B x 2^n of its workspace, any n the
        engine takes) and only the rows and the summary come back.  backend="host": the NumPy definition, n <= 24.
        An entry other than 0 / 1 raises ValueError("row i: ...") as seeding_forecasts does."""
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")
        return self._lattice_at(genotypes, "observation", backend, 3, self._metdist_host, self._metdist_device,
                                MetastasisDistribution, self._metdist_summary_host, MetastasisSummary)

    # ------------------------------------------------------------------ genotype distribution of one tumour given the other
    def _partner_rates(self):
        """What _partner_host needs of the model, formed once for any number of queries."""
        n, size = self.n, 1 << self.n
        idx, level, lam, sig = self._lattice_host_rates("distribution")
        mu = [lam[j] * np.exp(self.log_theta[j, n]) for j in range(n)]
        kap0 = np.exp(_subset_sums(self.obs1[:n]))
        kap1 = kap0 * np.exp(self.obs1[n])
        kapm = np.exp(self.obs2[n] + _subset_sums(self.obs2[:n]))
        L, Lm = np.zeros(size), np.zeros(size)
        for j in range(n):
            free = (idx >> j & 1) == 0
            L += np.where(free, lam[j], 0.0)
            Lm += np.where(free, mu[j], 0.0)
        chains = {"PT": (lam, kap1, L + kap1), "MT": (mu, kapm, Lm + kapm)}
        return idx, level, lam, sig, L + sig + kap0, chains

    def _partner_host(self, q: int, given: str, rates=None) -> np.ndarray:
        """[2, 2^n]: the definition of the partner distribution (W, J) of the query code q, level by level."""
        n, size = self.n, 1 << self.n
        idx, level, lam, sig, den0, chains = rates if rates is not None else self._partner_rates()
        (rq, kq, dq), (rp, kp, dp) = chains[given], chains["MT" if given == "PT" else "PT"]
        sub = (idx & ~q) == 0
        top = bin(q).count("1")
        F0, G0, B = (np.zeros(size) for _ in range(3))
        F0[0] = 1.0
        for lev in range(top + 1):                           # G0 on the subsets of q
            ys = idx[(level == lev) & sub]
            for b in range(n if lev else 0):
                to = ys[(ys >> b & 1) == 1]
                frm = to ^ (1 << b)
                F0[to] += G0[frm] * lam[b][frm]
            G0[ys] = F0[ys] / den0[ys]
        B[q] = kq[q] / dq[q]
        for lev in range(top - 1, -1, -1):                   # B: from a subset to q, then q's own clock
            xs = idx[(level == lev) & sub]
            num = np.zeros(len(xs))
            for j in range(n):
                if q >> j & 1:
                    m = (xs >> j & 1) == 0
                    x = xs[m]
                    num[m] += rq[j][x] * B[x | 1 << j]
            B[xs] = num / dq[xs]
        W = np.where(sub, sig * G0 * B, 0.0)
        F, G = W.copy(), np.zeros(size)
        for lev in range(n + 1):                             # the partner's chain from every founder at once
            ys = idx[level == lev]
            for b in range(n if lev else 0):
                to = ys[(ys >> b & 1) == 1]
                frm = to ^ (1 << b)
                F[to] += G[frm] * rp[b][frm]
            G[ys] = F[ys] / dp[ys]
        return np.stack((W, kp * G))

    @staticmethod
    def _partner_summary_host(P: np.ndarray) -> "PartnerSummary":
        """The PartnerSummary of the planes P [2, 2^n], by its definition."""
        s = MetMHN._genodist_summary_host(P)
        return PartnerSummary(s.mass, s.pairs, s.burden)

    def _lattice_max_bytes(self, max_bytes, planes, noun, prep, at):
        """_lattice_whole's refusal of a result of `planes` values per genotype that exceeds max_bytes."""
        n = self.n
        if 8 * planes << n > max_bytes:
            raise ValueError(f"{n} mutations: a {noun} {prep} 2^{n} genotypes needs {8 * planes << n} bytes, more than max_bytes = "
                             f"{int(max_bytes)}; {at} reads single genotypes off the device's {noun}")

    def _partner_checks(self, given, backend):
        if given not in _PARTNER_GIVEN:
            raise ValueError("given must be 'PT' or 'MT'")
        if backend not in ("device", "host"):
            raise ValueError("backend must be 'device' or 'host'")

    def partner_distribution(self, genotype, given: str = "PT", backend: str = "device",
                             max_bytes: int = 2 ** 31) -> "PartnerDistribution":
        """The distribution of the tumour that was NOT sequenced: for a primary tumour that has seeded and is observed with
        `genotype` [n] (0 / 1; given="PT") the joint probability with every genotype of its metastasis, for a metastasis
        observed with `genotype` (given="MT") the joint probability with every genotype of the primary tumour - one row or
        column of the (PT x MT) table, exp(lp) of the paired row (type 3) of unknown order for all 2^n partners at once.
        After the seeding the two tumours are independent chains, each stopped by its own clock, so the joint factorises
        through the founder z.  With metastasis_distribution's lambda, sigma, kappa0, mu, kappam, L, Lm, G0 and
        kappa1 = kappa0 exp(obs1_n), den1 = L + kappa1, denm = Lm + kappam, for given="PT" and the query x:
            B(x) = kappa1(x) / den1(x),  B(z) = sum_{j in x - z} lambda_j(z) B(z + j) / den1(z)    (z a subset of x; L in
                                                                             den1 over ALL mutations z lacks)
            W(z) = sigma(z) G0(z) B(z) on the subsets of x, 0 elsewhere      = P(founder z, PT observed seeded as x)
            FM(y) = W(y) + sum_b GM(y - b) mu_b(y - b),  GM = FM / denm,  J(y) = kappam(y) GM(y) = P(PT = x seeded, MT = y)
        and for given="MT" with the chains exchanged (B with mu, kappam, denm; the forward pass with lambda, kappa1, den1).
        `founder` = W, `partner` = J, `mass` = sum J = sum W = genotype_distribution().seeded[x] or
        metastasis_distribution().metastasis[y]; `conditional` and `founder_conditional` are the planes over `mass` (NaN
        when it is 0, the joints then being exact zeros); `summary` the PartnerSummary.

        backend="device": one call of the HIP library (mmhn_partner_distributions), 16 B x 2^n of workspace and as much here
        for the result; a ValueError names the bytes when that exceeds `max_bytes` (2 GiB: n <= 27).  backend="host": the
        definition in NumPy, level by level, n <= 24."""
        self._partner_checks(given, backend)
        n = self.n
        g = np.asarray(genotype)
        if g.ndim != 1:
            raise ValueError(f"genotype must have shape [{n}]")
        g = self._forecast_checks(g[None, :], "observation")
        q = int(g[0] @ (1 << np.arange(n, dtype=np.int64)))
        if backend == "host" and n > _LATTICE_HOST_MAX:
            self._lattice_host_rates("distribution")         # (raises: the message points to the device)
        self._lattice_max_bytes(max_bytes, 2, "distribution", "over", "partner_distributions")
        if backend == "host":
            whole = self._partner_host(q, given)
            summary, mass = self._partner_summary_host(whole), whole[1].sum()
        else:
            from .jx import engine
            values, _, sums, whole = engine(n).partner_distributions(self.log_theta, self.obs1, self.obs2, g.astype(np.int8),
                                                                     given, summary=True, full=True)
            summary, mass = PartnerSummary(*(s[0] for s in sums)), values[0, 0]
        return PartnerDistribution(whole[0], whole[1], np.arange(1 << n), float(mass), summary, given, q)

    def partner_distributions(self, genotypes, given: str = "PT", targets=None, backend: str = "device") -> SimpleNamespace:
        """partner_distribution of every row of `genotypes` [R, n] (0 / 1) without the planes: `mass` [R], `summaries` (a
        list of R PartnerSummary), `codes` [R] and, with `targets` [R, n], the joint `at_target` [R] with that genotype of
        the other tumour - exp(lp) of the paired row of unknown order - and `founder_at_target` [R], the joint with that
        founder (both NaN without targets).  Distinct genotypes are solved once.  backend="device": one call of the HIP
        library, 16 B x 2^n of its workspace, any n the engine takes; backend="host": the NumPy definition, n <= 24.  An
        entry other than 0 / 1 raises ValueError("row i: ...") as seeding_forecasts does."""
        self._partner_checks(given, backend)
        n = self.n
        g = self._forecast_checks(genotypes, "observation")
        t = None
        if targets is not None:
            if np.asarray(targets).shape != g.shape:
                raise ValueError(f"targets must have shape [R, {n}], a row per genotype")
            t = self._forecast_checks(targets, "observation")
        pw = 1 << np.arange(n, dtype=np.int64)
        codes = g @ pw
        R = len(codes)
        if backend == "host":
            rates = self._partner_rates()
            mass, at, fat, summaries = np.empty(R), np.full(R, np.nan), np.full(R, np.nan), [None] * R
            uniq, inverse = np.unique(codes, return_inverse=True)
            for k, q in enumerate(uniq):
                whole = self._partner_host(int(q), given, rates)
                summary = self._partner_summary_host(whole)
                for i in np.flatnonzero(inverse == k):
                    mass[i], summaries[i] = whole[1].sum(), summary
                    if t is not None:
                        fat[i], at[i] = whole[:, int(t[i] @ pw)]
        else:
            from .jx import engine
            values, status, sums, _ = engine(n).partner_distributions(
                self.log_theta, self.obs1, self.obs2, g.astype(np.int8), given,
                None if t is None else t.astype(np.int8), summary=True)
            bad = np.flatnonzero(status != 0)
            if bad.size:
                raise ValueError(f"row {int(bad[0])}: a genotype entry is neither 0 nor 1")
            mass, fat, at = (np.ascontiguousarray(values[:, k]) for k in range(3))
            summaries = [PartnerSummary(sums[0][i], sums[1][i], sums[2][i]) for i in range(R)]
        return SimpleNamespace(mass=mass, at_target=at, founder_at_target=fat, codes=codes, summaries=summaries, given=given)

    def likelihood(self, order, met_status: str, first_obs: str = None) -> float:
        """model.py:295-376: probability of exactly this order of events being what is observed."""
        order = tuple(int(e) for e in order)
        seeding = 2 * self.n
        if met_status == "isMetastasis":
            if any(e % 2 == 0 and e != seeding for e in order):
                raise ValueError("PT event in order, but met_status is 'isMetastasis'.")
            if seeding not in order:
                raise ValueError("Seeding event not in order, but met_status is 'isMetastasis'.")
            return self._likelihood_unpaired_mt(order)
        if met_status in ("absent", "present"):
            if any(e % 2 == 1 for e in order):
                raise ValueError(f"Met event in order, but met_status is '{met_status}'.")
            if met_status == "absent" and seeding in order:
                raise ValueError("Seeding event in order, but met_status is 'absent'.")
            if met_status == "present" and seeding not in order:
                raise ValueError("Seeding event not in order, but met_status is 'present'.")
            return self._likelihood_unpaired_pt(order)
        if met_status == "isPaired":
            if first_obs not in _FIRST_OBS:
                raise ValueError(_FIRST_ERR)
            if first_obs == "sync":
                warnings.warn("Synchronous development is deprecated.", DeprecationWarning)
            return self._likelihood_paired(order, first_obs)
        raise ValueError(_STATUS_ERR)

    # ------------------------------------------------------------------ one tumour
    def _single_tables(self, theta, state: State, obs_after):
        """Lattice tables of a one-tumour chain over the n+1 events, restricted to `state`.
        The observation rate follows obs1 until the seeding is in and `obs_after` from then on."""
        ev = list(state)
        k = len(ev)
        t1, t2 = _subset_sums(self.obs1[ev]), _subset_sums(obs_after[ev])
        x = np.arange(1 << k)
        seeded = (x >> (k - 1) & 1).astype(bool) if self.n in state else np.zeros(1 << k, dtype=bool)
        diag = _single_diag(theta, self.n + 1, ev)
        den = np.where(seeded, np.exp(t2), np.exp(t1)) - diag
        num = [np.exp(_subset_sums(theta[e, ev])) for e in ev]
        final = np.exp(t2[-1] if seeded[-1] else t1[-1])
        return SimpleNamespace(ev=ev, k=k, den=den, num=num, final=final)

    @staticmethod
    def _single_walk(T, events) -> float:
        x, p = 0, 1.0 / T.den[0]
        for e in events:
            b = T.ev.index(e)
            if x >> b & 1:
                raise ValueError("an event occurs twice in the order")
            x |= 1 << b
            p *= T.num[b][x] / T.den[x]
        return float(p * T.final)

    @staticmethod
    def _single_viterbi(T):
        """Best path to every sub-state in index order (every predecessor has a smaller index)."""
        best = np.zeros(1 << T.k)
        last = np.zeros(1 << T.k, dtype=np.int64)
        best[0] = 1.0 / T.den[0]
        for x in range(1, 1 << T.k):
            top, arg = -1.0, -1
            for b in range(T.k):
                if x >> b & 1:
                    cand = best[x ^ (1 << b)] * T.num[b][x]
                    if cand > top:
                        top, arg = cand, b
            best[x], last[x] = top / T.den[x], arg
        x, rev = (1 << T.k) - 1, []
        while x:
            rev.append(T.ev[last[x]])
            x ^= 1 << last[x]
        return np.array(rev[::-1], dtype=np.int64), float(best[-1] * T.final)

    def _posterior_single(self, T) -> "OrderPosterior":
        """_single_viterbi's recurrence with the maximum replaced by the sum, and its transpose over the seeded half."""
        n, k, V = self.n, T.k, 1 << T.k
        F = [0.0] * V
        F[0] = 1.0 / T.den[0]
        for x in range(1, V):
            s = 0.0
            for b in range(k):
                if x >> b & 1:
                    s += F[x ^ 1 << b] * T.num[b][x]
            F[x] = s / T.den[x]
        Z = F[-1] * T.final
        pre, pos = np.full(n, np.nan), np.full(n + 1, np.nan)
        if k == 0 or T.ev[-1] != n:                  # "absent": no seeding in the observation
            return OrderPosterior(float(np.log(Z)), pre, pos)
        top, full = 1 << (k - 1), V - 1
        B = {full: T.final}
        for x in range(full - 1, top - 1, -1):
            s = 0.0
            for b in range(k - 1):
                if not x >> b & 1:
                    y = x | 1 << b
                    s += B[y] * T.num[b][y] / T.den[y]
            B[x] = s
        pre[:], pos[:] = 0.0, 0.0
        for x in range(top):                         # the orders that seed at x
            y = x | top
            w = F[x] * T.num[k - 1][y] / T.den[y] * B[y]
            pos[bin(x).count("1")] += w
            for b in range(k - 1):
                if x >> b & 1:
                    pre[T.ev[b]] += w
        return OrderPosterior(float(np.log(Z)), pre / Z, pos / Z)

    def _precedence_matrix(self, codes, P, Z) -> np.ndarray:
        """The slot matrix P (summed move masses) over the evidence, at the positions of the slots' event codes."""
        prec = np.full((2 * self.n + 1, 2 * self.n + 1), np.nan)
        if len(codes):
            prec[np.ix_(codes, codes)] = np.minimum(P / Z, 1.0)     # the quotient of two roundings may pass 1
        return prec

    @staticmethod
    def _single_passes(T):
        """_posterior_single's forward pass F, the evidence Z and the backward pass over the whole lattice as
        G[x] = B[x] / den[x]: the move x -> y = x | d has the mass F[x] num_d[y] G[y]."""
        k, V = T.k, 1 << T.k
        F = np.zeros(V)
        F[0] = 1.0 / T.den[0]
        for x in range(1, V):
            s = 0.0
            for b in range(k):
                if x >> b & 1:
                    s += F[x ^ 1 << b] * T.num[b][x]
            F[x] = s / T.den[x]
        Z = F[-1] * T.final
        G = np.zeros(V)
        G[-1] = T.final / T.den[-1]
        for x in range(V - 2, -1, -1):
            s = 0.0
            for b in range(k):
                if not x >> b & 1:
                    y = x | 1 << b
                    s += G[y] * T.num[b][y]
            G[x] = s / T.den[x]
        return F, Z, G

    def _precedence_single(self, T, codes) -> "OrderPrecedence":
        """Per target slot d the masses of the moves x -> y = x | d (_single_passes), summed over the x that hold c."""
        k, V = T.k, 1 << T.k
        F, Z, G = self._single_passes(T)
        P = np.zeros((k, k))
        idx = np.arange(V)
        for d in range(k):
            xs = idx[(idx >> d & 1) == 0]
            w = F[xs] * T.num[d][xs | 1 << d] * G[xs | 1 << d]
            for c in range(k):
                if c != d:
                    P[c, d] = w[(xs >> c & 1) == 1].sum()
        return OrderPrecedence(float(np.log(Z)), self._precedence_matrix(codes, P, Z))

    def _position_single(self, T):
        """(log evidence, pos [n+1, n+1]) of a one-tumour chain: the masses of the moves that add slot d, summed by the
        number of events their state holds."""
        k, V = T.k, 1 << T.k
        F, Z, G = self._single_passes(T)
        pos = np.full((self.n + 1, self.n + 1), np.nan)
        idx = np.arange(V)
        held = np.array([bin(x).count("1") for x in range(V)])
        for d in range(k):
            xs = idx[(idx >> d & 1) == 0]
            w = F[xs] * T.num[d][xs | 1 << d] * G[xs | 1 << d]
            pos[T.ev[d]] = np.minimum(np.bincount(held[xs], weights=w, minlength=self.n + 1) / Z, 1.0)
        return float(np.log(Z)), pos

    def _time_single(self, T, codes) -> "OrderTime":
        """order_time on a one-tumour chain: h[x] = F[x] G[x] (_single_passes: F carries 1 / den[x], G = B / den) is the
        time the chain spends in x times the evidence; the event of slot d is still to come in the states without bit d."""
        k, V = T.k, 1 << T.k
        F, Z, G = self._single_passes(T)
        h = F * G
        idx = np.arange(V)
        time = np.full(2 * self.n + 1, np.nan)
        for d in range(k):
            time[codes[d]] = h[(idx >> d & 1) == 0].sum() / Z
        return OrderTime(float(np.log(Z)), time, np.array([h.sum() / Z, np.nan]), float("nan"))

    @staticmethod
    def _draw(W, u):
        """One move of every sample: W [M, C] the candidates' weights in visiting order (0: not a candidate), u [M] the
        uniforms.  Returns the candidate taken, its weight, the total and |u total - boundary| / total of the nearest
        boundary of a candidate with w > 0."""
        cum = np.add.accumulate(W, axis=1)                  # one after the other, as the kernel's loop
        total = cum[:, -1]
        t = u * total
        above = cum > t[:, None]
        last = W.shape[1] - 1 - np.argmax(W[:, ::-1] > 0.0, axis=1)
        pick = np.where(above.any(axis=1), np.argmax(above, axis=1), last)
        dist = np.where(W > 0.0, np.abs(cum - t[:, None]), np.inf).min(axis=1) / total
        return pick, W[np.arange(len(pick)), pick], total, dist

    def _sample_single(self, T, codes, samples, key, row) -> "OrderSample":
        """sample_order on a one-tumour chain: the weights of _single_passes' backward pass, move by move."""
        _, Z, G = self._single_passes(T)
        k, M = T.k, len(samples)
        codes = np.array(codes, dtype=np.int8)
        orders = np.full((M, 2 * self.n + 1), -1, dtype=np.int8)
        log_prob, margin, totals = np.zeros(M), np.full(M, np.inf), np.full((M, k), np.nan)
        x = np.zeros(M, dtype=np.int64)
        for move in range(k):
            W = np.zeros((M, k))
            for b in range(k):
                y = x | 1 << b
                W[:, b] = np.where(x >> b & 1, 0.0, T.num[b][y] * G[y])
            pick, w, total, dist = self._draw(W, _philox.order_uniforms(key, row, samples, move))
            orders[:, move] = codes[pick]
            log_prob += np.log(w / total)
            margin = np.minimum(margin, dist)
            totals[:, move] = total
            x |= 1 << pick
        return OrderSample(float(np.log(Z)), orders, log_prob, margin, totals)

    def _likelihood_unpaired_mt(self, order) -> float:
        """model.py:1391-1426: a metastasis seen once (obs2), the chain feeling the seeding."""
        events = [e // 2 for e in order]
        T = self._single_tables(self.log_theta, State(events, size=self.n + 1), self.obs2)
        return self._single_walk(T, events)

    def _likeliest_order_unpaired_mt(self, state: State):
        """model.py:448-501."""
        T = self._single_tables(self.log_theta, state, self.obs2)
        events, p = self._single_viterbi(T)
        codes = 2 * events + 1
        codes[events == self.n] = 2 * self.n
        return codes, p

    def _likelihood_unpaired_pt(self, order) -> float:
        """model.py:343,356: the reference hands these to mhn.oMHN(vstack(theta with the seeding's
        column zeroed, obs1)).order_likelihood -- a one-tumour chain over the n+1 events whose
        observation rate is exp(obs1 . state); expansion in the reference's tests/test_orders.py:76-100."""
        events = [e // 2 for e in order]
        T = self._single_tables(self._pt_log_theta, State(events, size=self.n + 1), self.obs1)
        return self._single_walk(T, events)

    def _likeliest_order_unpaired_pt(self, state: State):
        """model.py:260-274 (mhn.oMHN.likeliest_order on the same chain)."""
        T = self._single_tables(self._pt_log_theta, state, self.obs1)
        events, p = self._single_viterbi(T)
        return 2 * events, p

    # ------------------------------------------------------------------ both tumours
    def _paired_tables(self, state: MetState, first_obs: str):
        """Lattice tables over the 2^k sub-states of `state` (bit b = its b-th occupied slot)."""
        n, th = self.n, self.log_theta
        slots = list(state)
        k = len(slots)
        if not state.Seeding:
            raise ValueError("a paired sample needs the seeding event")
        kind = [2 if s == 2 * n else s & 1 for s in slots]            # 0 PT, 1 MT, 2 seeding
        ev = [n if s == 2 * n else s // 2 for s in slots]
        in_pt = [kd != 1 for kd in kind]                                # slots obs1 / PT rates look at
        in_mt = [kd != 0 for kd in kind]
        s1 = _subset_sums([self.obs1[e] if f else 0.0 for e, f in zip(ev, in_pt)])
        s2 = _subset_sums([self.obs2[e] if f else 0.0 for e, f in zip(ev, in_mt)])
        seeded = (np.arange(1 << k) >> (k - 1) & 1).astype(bool)
        o1, o2 = np.exp(s1), np.exp(s2)
        den = o1 + np.where(seeded, o2, 0.0) - self._get_diag_paired(state)
        # numerator of the event in slot b: its row of theta summed over the PT slots (a PT event;
        # before the seeding both tumours agree) or over the MT slots and the seeding (a metastasis
        # event, the seeding itself)  (model.py:1466-1503)
        def row(b):
            flags = [kd == 0 for kd in kind] if kind[b] == 0 else in_mt
            return np.exp(_subset_sums([th[ev[b], e] if f else 0.0 for e, f in zip(ev, flags)]))
        num = [row(b) for b in range(k)]
        T = SimpleNamespace(k=k, slots=slots, kind=kind, seeded=seeded, den=den, num=num, o1=o1, o2=o2,
                            pt_first=first_obs in ("PT", "unknown"), mt_first=first_obs in ("Met", "unknown"),
                            sync=first_obs == "sync",
                            pt_mask=sum(1 << b for b in range(k) if kind[b] == 0),
                            mt_mask=sum(1 << b for b in range(k) if kind[b] == 1),
                            joint=sum(1 << b for b in range(k - 1)
                                      if kind[b] == 0 and kind[b + 1] == 1 and ev[b] == ev[b + 1]))
        # the tumour that is left after the first observation runs on alone (model.py:1515-1536,
        # 1643-1663): the metastasis with the seeding's effects under obs2, or the primary tumour
        # without them under obs1 (which still counts the seeding)
        if T.pt_first:
            du = self._get_diag_unpaired(state.MT)
            T.den_mt = o2 - du[_subset_index(in_mt)]
        if T.mt_first:
            du = self._get_diag_unpaired(state.PT, seeding=False)
            T.den_pt = o1 - du[_subset_index([kd == 0 for kd in kind])]
        return T

    @staticmethod
    def _settle(T, x: int, v):
        """(a, b_P, b_M) with "the first observation happens now" folded into the b's, which is
        admissible once the seeding and every event of the first-observed tumour are in."""
        a, bp, bm = v
        if T.seeded[x]:
            if T.pt_first and x & T.pt_mask == T.pt_mask:
                bp = bp + a * T.o1[x] / T.den_mt[x]
            if T.mt_first and x & T.mt_mask == T.mt_mask:
                bm = bm + a * T.o2[x] / T.den_pt[x]
        return a, bp, bm

    @staticmethod
    def _advance(T, x: int, v, b: int):
        """Add the event in slot b (a joint event, slots b and b+1, before the seeding)."""
        if not T.seeded[x] and b != T.k - 1:
            y = x | 3 << b
            return y, (v[0] * T.num[b][y] / T.den[y], 0.0, 0.0)
        y = x | 1 << b
        a, bp, bm = MetMHN._settle(T, x, v)
        num = T.num[b][y]
        bp = bp * num / T.den_mt[y] if T.pt_first and T.kind[b] == 1 else 0.0
        bm = bm * num / T.den_pt[y] if T.mt_first and T.kind[b] == 0 else 0.0
        return y, (a * num / T.den[y], bp, bm)

    @staticmethod
    def _total(T, v) -> float:
        full = (1 << T.k) - 1
        a, bp, bm = MetMHN._settle(T, full, v)
        if T.sync:
            return float(a * (T.o1[full] + T.o2[full]))           # model.py:1746-1751
        return float(bp * T.o2[full] + bm * T.o1[full])

    def _likelihood_paired(self, order, first_obs: str) -> float:
        """model.py:1540-1553, 1667-1750: all admissible first-observation points summed."""
        if len(set(order)) != len(order):
            raise ValueError("an event occurs twice in the order")
        if 2 * self.n not in order:
            raise ValueError("Seeding event not in order, but met_status is 'isPaired'.")
        T = self._paired_tables(MetState(order, size=2 * self.n + 1), first_obs)
        x, v, i = 0, (1.0 / T.den[0], 0.0, 0.0), 0
        while i < len(order):
            b = T.slots.index(order[i])
            if not T.seeded[x] and b != T.k - 1:
                if not (T.joint >> b & 1 and i + 1 < len(order) and order[i + 1] == order[i] + 1):
                    raise ValueError("before the seeding an event must occur in both tumours (2i, 2i+1)")
                i += 1
            x, v = self._advance(T, x, v, b)
            i += 1
        return self._total(T, v)

    def _paired_passes(self, state: MetState, first_obs: str):
        """The two sum-product passes of a paired row: tables T, forward prefix vectors F (unsettled, every state the
        chain can be in), evidence Z, backward weights B over the seeded half (B[x] is the weight the rest of the order
        gives the unsettled vector at x)."""
        if not state.reachable:
            raise ValueError("This state is not reachable by mhn.")
        T = self._paired_tables(state, first_obs)
        n, k = self.n, T.k
        top, full = 1 << (k - 1), (1 << k) - 1
        F = {0: (1.0 / T.den[0], 0.0, 0.0)}
        for y in range(1, 1 << k):
            if not y & top:
                lo = y & T.joint
                if y != lo | lo << 1:
                    continue                                    # tumours differ before the seeding
                moves = [(y ^ 3 << b, b) for b in range(k - 1) if lo >> b & 1]
            else:
                moves = [(y ^ 1 << b, b) for b in range(k) if y >> b & 1 and y ^ 1 << b in F]
            a = bp = bm = 0.0
            for x, b in moves:
                v = self._advance(T, x, F[x], b)[1]
                a, bp, bm = a + v[0], bp + v[1], bm + v[2]
            F[y] = (a, bp, bm)
        Z = self._total(T, F[full])

        def settle_t(x, ga, gp, gm):                            # _settle transposed (x seeded)
            if T.pt_first and x & T.pt_mask == T.pt_mask:
                ga = ga + gp * (T.o1[x] / T.den_mt[x])
            if T.mt_first and x & T.mt_mask == T.mt_mask:
                ga = ga + gm * (T.o2[x] / T.den_pt[x])
            return ga, gp, gm

        t = (T.o1[full] + T.o2[full], 0.0, 0.0) if T.sync else (0.0, T.o2[full], T.o1[full])
        B = {full: settle_t(full, *t)}
        for x in range(full - 1, top - 1, -1):
            ga = gp = gm = 0.0
            for b in range(k - 1):
                if not x >> b & 1:
                    y = x | 1 << b
                    num, g = T.num[b][y], B[y]
                    ga += g[0] * num / T.den[y]
                    if T.pt_first and T.kind[b] == 1:
                        gp += g[1] * num / T.den_mt[y]
                    if T.mt_first and T.kind[b] == 0:
                        gm += g[2] * num / T.den_pt[y]
            B[x] = settle_t(x, ga, gp, gm)
        return T, F, Z, B

    def _posterior_paired(self, state: MetState, first_obs: str) -> "OrderPosterior":
        """_likeliest_order_paired's walk with the Pareto step replaced by the sum (_advance, _settle and _total are
        linear in the prefix vector), then the transposed walk over the seeded half: B[x] is the weight the rest of the
        order gives the (unsettled) vector at x, so the orders that seed at x have the mass B[x | top] . A(x, top) F[x]."""
        T, F, Z, B = self._paired_passes(state, first_obs)
        n, k = self.n, T.k
        top = 1 << (k - 1)
        pre, pos = np.zeros(n), np.zeros(n + 1)
        for x in F:
            if x & top:
                continue
            y = x | top
            w = B[y][0] * (F[x][0] * T.num[k - 1][y] / T.den[y])
            pos[bin(x).count("1") // 2] += w
            for b in range(k - 1):
                if T.joint >> b & 1 and x >> b & 1:
                    pre[T.slots[b] // 2] += w
        return OrderPosterior(float(np.log(Z)), pre / Z, pos / Z)

    @staticmethod
    def _unseeded_backward(T, F, B) -> dict:
        """_paired_passes' backward pass continued over the unseeded states whose tumours agree: a scalar per state (joint
        moves and the seeding edge), the weight the rest of the order gives F[x]_a."""
        k = T.k
        top = 1 << (k - 1)
        Bu = {}
        for x in sorted((x for x in F if not x & top), reverse=True):
            y = x | top
            s = 0.0
            for b in range(k - 1):
                if T.joint >> b & 1 and not x >> b & 1:
                    s += T.num[b][x | 3 << b] / T.den[x | 3 << b] * Bu[x | 3 << b]
            Bu[x] = s + T.num[k - 1][y] / T.den[y] * B[y][0]
        return Bu

    def _position_paired(self, state: MetState, first_obs: str) -> "OrderPosition":
        """_precedence_paired's move masses, added to the position popcount(x & the slots of the lineage) of the event the
        move adds; before the seeding both tumours agree and a state of j joint events puts the move's event at j in both
        lineages."""
        T, F, Z, B = self._paired_passes(state, first_obs)
        n, k = self.n, T.k
        top = 1 << (k - 1)
        Bu = self._unseeded_backward(T, F, B)
        ev = [n if s == 2 * n else s // 2 for s in T.slots]
        count = lambda x: bin(x).count("1")
        pos_pt, pos_mt = np.full((n + 1, n + 1), np.nan), np.full((n + 1, n + 1), np.nan)
        for d in range(k):
            if T.kind[d] != 1:
                pos_pt[ev[d]] = 0.0
            if T.kind[d] != 0:
                pos_mt[ev[d]] = 0.0
        for x in F:
            if x & top:
                for d in range(k - 1):
                    if not x >> d & 1:
                        y, v = self._advance(T, x, F[x], d)
                        g = B[y]
                        w = g[0] * v[0] + g[1] * v[1] + g[2] * v[2]
                        if T.kind[d] == 0:
                            pos_pt[ev[d], count(x & (T.pt_mask | top))] += w
                        else:
                            pos_mt[ev[d], count(x & (T.mt_mask | top))] += w
                continue
            j = count(x) // 2
            y = x | top
            w = B[y][0] * (F[x][0] * T.num[k - 1][y] / T.den[y])
            pos_pt[n, j] += w
            pos_mt[n, j] += w
            for b in range(k - 1):
                if T.joint >> b & 1 and not x >> b & 1:
                    y = x | 3 << b
                    w = F[x][0] * T.num[b][y] / T.den[y] * Bu[y]
                    pos_pt[ev[b], j] += w
                    pos_mt[ev[b], j] += w
        return OrderPosition(float(np.log(Z)), np.minimum(pos_pt / Z, 1.0), np.minimum(pos_mt / Z, 1.0))

    def _time_paired(self, state: MetState, first_obs: str) -> "OrderTime":
        """order_time on a paired row: _paired_passes and _unseeded_backward, then per state the time the chain spends
        there times the evidence - hu before the seeding, ha after it with no observation made yet, hb with the first
        observation made and the other tumour running on alone under its own den - added to every slot the state does not
        hold yet."""
        T, F, Z, B = self._paired_passes(state, first_obs)
        Bu = self._unseeded_backward(T, F, B)
        k = T.k
        top, full = 1 << (k - 1), (1 << k) - 1
        slot = [0.0] * k
        su = sa = sb = 0.0
        for x in sorted(F):
            if not x & top:
                h = F[x][0] * Bu[x] / T.den[x]
                su += h
            else:
                _, bp, bm = self._settle(T, x, F[x])
                g = B[x]
                ha = F[x][0] * g[0] / T.den[x]
                hb = 0.0
                if T.pt_first:
                    hb += bp * g[1] / T.den_mt[x]
                if T.mt_first:
                    hb += bm * g[2] / T.den_pt[x]
                sa += ha
                sb += hb
                h = ha + hb
            for d in range(k):
                if not x >> d & 1:
                    slot[d] += h
        time = np.full(2 * self.n + 1, np.nan)
        time[T.slots] = np.array(slot) / Z
        first = su + sa
        pt_first = float("nan") if T.sync else float(self._settle(T, full, F[full])[1] * T.o2[full] / Z)
        return OrderTime(float(np.log(Z)), time, np.array([first / Z, (first + sb) / Z]), pt_first)

    def _snapshot_none(self, log_evidence: float) -> "OrderSnapshot":
        """order_snapshot of an observation without a first observation."""
        L = 2 * self.n + 1
        return OrderSnapshot(log_evidence, np.full((2, L), np.nan), np.full((2, self.n + 1), np.nan),
                             np.full(L, -1, dtype=np.int8), -1, float("nan"))

    def _snapshot_paired(self, state: MetState, first_obs: str) -> "OrderSnapshot":
        """order_snapshot on a paired row: _paired_passes, then per regime r the masses of the seeded states that hold every
        slot of the first-observed tumour, added to every slot the state holds and to the number of slots it lacks; the
        largest mass is kept, the first of equal ones in the order (r, x)."""
        T, F, Z, B = self._paired_passes(state, first_obs)
        le = float(np.log(Z))
        if T.sync:
            return self._snapshot_none(le)
        n, k = self.n, T.k
        top, full = 1 << (k - 1), (1 << k) - 1
        slot, late = np.zeros((2, k)), np.zeros((2, n + 1))
        best = (-1.0, -1, 0)
        regimes = ((T.pt_first, T.pt_mask, T.o1, getattr(T, "den_mt", None), 1),
                   (T.mt_first, T.mt_mask, T.o2, getattr(T, "den_pt", None), 2))
        for r, (possible, own, o, den, comp) in enumerate(regimes):
            if not possible:
                continue
            for x in range(top, full + 1):
                if x & own != own:
                    continue
                s = F[x][0] * o[x] / den[x] * B[x][comp]
                for d in range(k):
                    if x >> d & 1:
                        slot[r, d] += s
                late[r, bin(full ^ x).count("1")] += s
                if s > best[0]:
                    best = (s, r, x)
        held = np.full((2, 2 * n + 1), np.nan)
        held[:, T.slots] = np.minimum(slot / Z, 1.0)             # the quotient of two roundings may pass 1
        map_state = np.full(2 * n + 1, -1, dtype=np.int8)
        map_state[T.slots] = [best[2] >> d & 1 for d in range(k)]
        return OrderSnapshot(le, held, np.minimum(late / Z, 1.0), map_state, best[1], float(min(best[0] / Z, 1.0)))

    def _precedence_paired(self, state: MetState, first_obs: str) -> "OrderPrecedence":
        """_posterior_paired's passes, the backward pass continued over the unseeded states whose tumours agree (a scalar:
        joint moves and the seeding edge), and the mass of EVERY move added to P[c, d] for the slots c its state holds and
        the slot(s) d it adds - a joint move adds both of its slots, so neither precedes the other."""
        T, F, Z, B = self._paired_passes(state, first_obs)
        k = T.k
        top = 1 << (k - 1)
        bits = lambda x: [c for c in range(k) if x >> c & 1]
        P = np.zeros((k, k))
        Bu = self._unseeded_backward(T, F, B)
        for x in F:
            held = bits(x)
            if x & top:
                for d in range(k - 1):
                    if not x >> d & 1:
                        y, v = self._advance(T, x, F[x], d)
                        g = B[y]
                        w = g[0] * v[0] + g[1] * v[1] + g[2] * v[2]
                        for c in held:
                            P[c, d] += w
                continue
            y = x | top
            w = B[y][0] * (F[x][0] * T.num[k - 1][y] / T.den[y])
            for c in held:
                P[c, k - 1] += w
            for b in range(k - 1):
                if T.joint >> b & 1 and not x >> b & 1:
                    y = x | 3 << b
                    w = F[x][0] * T.num[b][y] / T.den[y] * Bu[y]
                    for c in held:
                        P[c, b] += w
                        P[c, b + 1] += w
        return OrderPrecedence(float(np.log(Z)), self._precedence_matrix(T.slots, P, Z))

    def _sample_paired(self, state: MetState, first_obs: str, samples, key, row) -> "OrderSample":
        """sample_order on a paired row: _unseeded_backward's terms before the seeding, then the three terms of a seeded
        move's mass (_precedence_paired) with the path's own prefix vector in F's place."""
        T, F, Z, B = self._paired_passes(state, first_obs)
        Bu = self._unseeded_backward(T, F, B)
        k, M = T.k, len(samples)
        top, full = 1 << (k - 1), (1 << k) - 1
        Ba, Bua = np.zeros((1 << k, 3)), np.zeros(1 << k)
        Ba[list(B)] = list(B.values())
        Bua[list(Bu)] = list(Bu.values())
        jslot = np.array([b for b in range(k - 1) if T.joint >> b & 1], dtype=np.int64)
        kj = len(jslot)
        slots = np.array(T.slots, dtype=np.int8)
        orders = np.full((M, 2 * self.n + 1), -1, dtype=np.int8)
        log_prob, margin, totals = np.zeros(M), np.full(M, np.inf), np.full((M, k), np.nan)
        x, held = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
        f = np.zeros((M, 3))
        move = 0
        while M and (x != full).any():
            u = _philox.order_uniforms(key, row, samples, move)
            before, after = np.flatnonzero(x < top), np.flatnonzero((x >= top) & (x != full))
            if before.size:
                xs = x[before]
                W = np.zeros((before.size, kj + 1))
                for q, b in enumerate(jslot):
                    y = xs | 3 << b
                    W[:, q] = np.where(xs >> b & 1, 0.0, T.num[b][y] / T.den[y] * Bua[y])
                y = xs | top
                W[:, kj] = T.num[k - 1][y] / T.den[y] * Ba[y, 0]
                pick, w, total, dist = self._draw(W, u[before])
                log_prob[before] += np.log(w / total)
                margin[before] = np.minimum(margin[before], dist)
                totals[before, move] = total
                jm = pick < kj
                a, b = before[jm], jslot[pick[jm]] if kj else pick[jm]
                orders[a, held[a]], orders[a, held[a] + 1] = slots[b], slots[b + 1]      # the PT code, then the MT code
                held[a] += 2
                x[a] |= 3 << b
                a = before[~jm]
                orders[a, held[a]] = slots[k - 1]
                held[a] += 1
                x[a] |= top
                f[a] = 0.0
                f[a, 0] = 1.0 / Ba[x[a], 0]
            if after.size:
                xs = x[after]
                fa, fp, fm = f[after].T
                if T.pt_first:                                              # _settle
                    fp = np.where(xs & T.pt_mask == T.pt_mask, fp + fa * T.o1[xs] / T.den_mt[xs], fp)
                if T.mt_first:
                    fm = np.where(xs & T.mt_mask == T.mt_mask, fm + fa * T.o2[xs] / T.den_pt[xs], fm)
                W, g = np.zeros((after.size, k - 1)), np.zeros((after.size, k - 1, 3))
                for b in range(k - 1):
                    y = xs | 1 << b
                    num = T.num[b][y]
                    g[:, b, 0] = fa * num / T.den[y]
                    w = Ba[y, 0] * g[:, b, 0]
                    if T.pt_first and T.kind[b] == 1:
                        g[:, b, 1] = fp * num / T.den_mt[y]
                        w = w + Ba[y, 1] * g[:, b, 1]
                    if T.mt_first and T.kind[b] == 0:
                        g[:, b, 2] = fm * num / T.den_pt[y]
                        w = w + Ba[y, 2] * g[:, b, 2]
                    W[:, b] = np.where(xs >> b & 1, 0.0, w)
                pick, w, total, dist = self._draw(W, u[after])
                log_prob[after] += np.log(w / total)
                margin[after] = np.minimum(margin[after], dist)
                totals[after, move] = total
                f[after] = g[np.arange(after.size), pick] / w[:, None]
                orders[after, held[after]] = slots[pick]
                held[after] += 1
                x[after] |= 1 << pick
            move += 1
        return OrderSample(float(np.log(Z)), orders, log_prob, margin, totals)

    def _likeliest_order_paired(self, state: MetState, first_obs: str):
        """model.py:503-1389 (_likeliest_order_pt_mt / _mt_pt / _unknown / _sync)."""
        if not state.reachable:
            raise ValueError("This state is not reachable by mhn.")
        T = self._paired_tables(state, first_obs)
        k, top = T.k, 1 << (T.k - 1)
        # front[x]: candidates (vector, predecessor candidate, slot, joint event?) nobody dominates
        front = {0: [((1.0 / T.den[0], 0.0, 0.0), None, -1, False)]}
        for y in range(1, 1 << k):
            cands = []
            if not y & top:
                lo = y & T.joint
                if y != lo | lo << 1:
                    continue                                    # tumours differ before the seeding
                for b in range(k - 1):
                    if lo >> b & 1:
                        x = y ^ 3 << b
                        cands.extend((self._advance(T, x, c[0], b)[1], c, b, True) for c in front[x])
                front[y] = [max(cands, key=lambda c: c[0][0])]
                continue
            for b in range(k):
                x = y ^ 1 << b
                if y >> b & 1 and x in front:
                    cands.extend((self._advance(T, x, c[0], b)[1], c, b, False) for c in front[x])
            keep = _pareto([self._settle(T, y, c[0]) for c in cands])
            front[y] = [cands[i] for i in keep]
        best = max(front[(1 << k) - 1], key=lambda c: self._total(T, c[0]))
        rev, c = [], best
        while c[1] is not None:
            rev.extend([T.slots[c[2] + 1], T.slots[c[2]]] if c[3] else [T.slots[c[2]]])
            c = c[1]
        return tuple(int(s) for s in rev[::-1]), self._total(T, best[0])
