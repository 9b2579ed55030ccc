"""What MetMHN's entry points return: the result containers of the order family (OrderPosterior(s) ... OrderSamples), of
the forecast and the landscape (SeedingForecast(s), SeedingLandscape) and of the three genotype distributions with their
exact summaries (GenotypeSummary, MetastasisSummary, PartnerSummary and the strata tuples), of the exact second moments
of the paired table (CrossSummary, PairedSummary), and the cohort statistics computed from them.  NumPy only: nothing here touches the model or the device.  model.py fills the containers (from the
HIP library or from order_host.py / lattice_host.py) and re-exports every name; simulations.PairSummary.compare shares
_residuals, and _entry_times serves OrderSamples' two sample means."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np


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


def _residuals(counts, rows, p) -> np.ndarray:
    """The standardised residuals (counts - rows p) / sqrt(rows p (1 - p)) of observed counts against `rows` draws with
    the frequencies p; NaN where p is not inside (0, 1).  The three compare methods share it: GenotypeSummary's,
    MetastasisSummary's and simulations.PairSummary's."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (counts - rows * p) / np.sqrt(rows * p * (1.0 - p))
    r[~((p > 0.0) & (p < 1.0))] = np.nan
    return r


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

    _STRATA = GENOTYPE_STRATA                    # a subclass names its own planes here

    def __repr__(self):
        return f"{type(self).__name__}(n_mut={self.n_mut}, mass={self.mass.tolist()})"

    def _stratum(self, stratum):
        """(pair sums [n, n], burden sums [n+1], mass) of a stratum."""
        if stratum not in self._STRATA:
            raise ValueError(f"stratum must be one of {self._STRATA}, got {stratum!r}")
        if stratum == "unknown":
            return self.pairs[0] + self.pairs[1], self.burden[0] + self.burden[1], self.mass[0] + self.mass[1]
        s = self._STRATA.index(stratum)
        return self.pairs[s], self.burden[s], self.mass[s]

    def _pair_counts(self, dat):
        """compare's `dat` as an array behind its shape check, with Utilityfunctions.pair_counts of it."""
        from .Utilityfunctions import pair_counts
        dat = np.asarray(dat)
        if dat.ndim != 2 or dat.shape[1] != 2 * self.n_mut + 3:
            raise ValueError(f"dat must have shape (n_pat, {2 * self.n_mut + 3}), got {dat.shape}")
        return (dat,) + tuple(pair_counts(dat))

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
        dat, n_type, obs = self._pair_counts(dat)
        g4 = dat[dat[:, -1] == 4][:, 0:2 * self.n_mut:2].astype(np.int64)
        seen = {"NM": (int(n_type[0]), obs[0][0::2, 0::2]), "EM-PT": (int(n_type[1]), obs[1][0::2, 0::2]),
                "unknown": (g4.shape[0], g4.T @ g4)}
        return {stratum: _residuals(counts, rows, self.frequencies(stratum))
                for stratum, (rows, counts) in seen.items() if rows}


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

    _STRATA = METASTASIS_STRATA

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
        _, n_type, obs = self._pair_counts(dat)
        p = self.frequencies("MT")
        return {key: _residuals(obs[t][1::2, 1::2], int(n_type[t]), p)
                for key, t in (("EM-MT", 2), ("paired", 3)) if n_type[t]}


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


class PartnerSummary(GenotypeSummary):
    """Exact sums over the joint distribution of one observed tumour with the founder (plane 0, W) and with the tumour
    that was not sequenced, the partner (plane 1, J), GenotypeSummary's arrays: mass [2] (the two are equal, the
    probability of the observed tumour's genotype), pairs [2, n, n], burden [2, n+1] - unnormalised, as in the siblings.
    Strata (PARTNER_STRATA): "founder" plane 0 over mass[0], "partner" plane 1 over mass[1]; frequencies, log_odds and
    burden_pmf are GenotypeSummary's and divide by the stratum's mass, so they are conditional on the observed tumour."""

    _STRATA = PARTNER_STRATA

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


def _log_odds(f, row, col) -> np.ndarray:
    """Log odds ratio of the 2x2 tables with joint frequency f [a, b] and marginal ones row [a], col [b]:
    log(p11 p00 / (p10 p01)); NaN where a cell is not positive (PairSummary's rule)."""
    p10, p01 = row[:, None] - f, col[None, :] - f
    p00 = 1.0 - row[:, None] - col[None, :] + f
    cells = np.stack((f, p10, p01, p00))
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.log(f) + np.log(p00) - np.log(p10) - np.log(p01)
    lo[~(cells > 0).all(axis=0)] = np.nan
    return lo


class CrossSummary:
    """The exact second moments of the (PT x MT) table of a seeded pair, all JOINT with "seeded" (the callers divide by
    `mass`): mass = P(seeded), pt [n] = P(PT holds i, seeded), mt [n] = P(MT holds j, seeded), cross [n, n] = P(PT holds i,
    MT holds j, seeded), burden [n+1, n+1] = P(|PT| = k, |MT| = l, seeded), gene_burden [2, n, n+1]: [0, i, l] = P(PT holds
    i, |MT| = l, seeded), [1, j, k] = P(MT holds j, |PT| = k, seeded).  What simulate_pairs estimates from samples in the
    PT x MT block of its "paired" stratum, without the sampling error.  MetMHN.cross_distribution fills it; with
    burden=False the last two are NaN."""

    def __init__(self, mass, pt, mt, cross, burden, gene_burden):
        self.mass = float(mass)
        self.pt = np.asarray(pt, dtype=np.float64).reshape(-1)
        self.n_mut = n = self.pt.shape[0]
        self.mt = np.asarray(mt, dtype=np.float64).reshape(n)
        self.cross = np.asarray(cross, dtype=np.float64).reshape(n, n)
        self.burden = np.asarray(burden, dtype=np.float64).reshape(n + 1, n + 1)
        self.gene_burden = np.asarray(gene_burden, dtype=np.float64).reshape(2, n, n + 1)

    def __repr__(self):
        return f"CrossSummary(n_mut={self.n_mut}, mass={self.mass})"

    def shared(self) -> np.ndarray:
        """[n]: the probability that both tumours of a seeded pair hold mutation i, diag(cross) / mass."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(self.cross) / np.float64(self.mass)

    def in_primary_given_metastasis(self) -> np.ndarray:
        """[n]: P(PT holds i | MT holds i, seeded) = diag(cross) / mt (NaN where mt is 0)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(self.cross) / self.mt

    def in_metastasis_given_primary(self) -> np.ndarray:
        """[n]: P(MT holds i | PT holds i, seeded) = diag(cross) / pt (NaN where pt is 0)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(self.cross) / self.pt

    def expected_shared(self) -> float:
        """The expected number of mutations both tumours of a seeded pair hold, trace(cross) / mass."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.trace(self.cross) / np.float64(self.mass))

    def frequencies(self) -> np.ndarray:
        """cross / mass [n, n]: [i, j] the probability that the PT of a seeded pair holds i and its MT holds j."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.cross / np.float64(self.mass)

    def burden_pmf(self) -> np.ndarray:
        """burden / mass [n+1, n+1]: the joint distribution of the two tumours' mutation counts of a seeded pair."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.burden / np.float64(self.mass)

    def log_odds(self) -> np.ndarray:
        """[n, n]: log odds ratio of (i in PT, j in MT) of a seeded pair from its 2x2 table, log(p11 p00 / (p10 p01)) with
        p11 = cross / mass and the other cells from pt / mass and mt / mass; NaN where a cell is not positive."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return _log_odds(self.frequencies(), self.pt / np.float64(self.mass), self.mt / np.float64(self.mass))


PAIRED_STRATA = ("paired",)                     # the one stratum of a PairedSummary: cohort rows of type 3


class PairedSummary:
    """The exact pairwise frequencies of a seeded pair over the 2 n columns [PT_0, MT_0, PT_1, MT_1, ...] of
    simulations.PairSummary - the exact form of simulate_pairs(...).frequencies("paired"): the PT x PT block from
    `primary` (GenotypeSummary, plane 1 over its mass), MT x MT from `metastasis` (MetastasisSummary, plane 1 over its
    mass), PT x MT from `cross` (CrossSummary, over its mass); [2i, 2i+1] = mutation i in both tumours.
    MetMHN.paired_summary fills it."""

    def __init__(self, primary, metastasis, cross):
        self.primary, self.metastasis, self.cross = primary, metastasis, cross
        self.n_mut = n = cross.n_mut
        self.mass = cross.mass
        f = np.empty((2 * n, 2 * n))
        f[0::2, 0::2] = primary.frequencies("EM-PT")
        f[1::2, 1::2] = metastasis.frequencies("MT")
        f[0::2, 1::2] = cross.frequencies()
        f[1::2, 0::2] = cross.frequencies().T
        self._frequencies = f

    def __repr__(self):
        return f"PairedSummary(n_mut={self.n_mut}, mass={self.mass})"

    def _stratum(self, stratum):
        if stratum not in PAIRED_STRATA:
            raise ValueError(f"stratum must be one of {PAIRED_STRATA}, got {stratum!r}")

    def frequencies(self, stratum="paired") -> np.ndarray:
        """[2n, 2n]: joint frequencies of two columns of a seeded pair, marginal ones on the diagonal."""
        self._stratum(stratum)
        return self._frequencies.copy()

    def log_odds(self, stratum="paired") -> np.ndarray:
        """Log odds ratio of every two columns from their 2x2 table; NaN where a cell is not positive (the diagonal
        included)."""
        f = self.frequencies(stratum)
        return _log_odds(f, np.diag(f), np.diag(f))

    def compare(self, dat) -> dict:
        """The exact form of simulate_pairs(...).compare(dat)["paired"]: {"paired": residuals [2n, 2n]} - the standardised
        residuals (obs - rows p) / sqrt(rows p (1 - p)) of the type-3 rows' Utilityfunctions.pair_counts against
        p = frequencies("paired"), NaN where p is not inside (0, 1); {} for a cohort without paired rows."""
        from .Utilityfunctions import pair_counts
        dat = np.asarray(dat)
        if dat.ndim != 2 or dat.shape[1] != 2 * self.n_mut + 3:
            raise ValueError(f"dat must have shape (n_pat, {2 * self.n_mut + 3}), got {dat.shape}")
        n_type, obs = pair_counts(dat)
        return {"paired": _residuals(obs[3], np.float64(n_type[3]), self.frequencies("paired"))} if n_type[3] else {}
