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

Where things are.  This file holds class MetMHN: the constructor, the two diagonals, the routing of an observation
(_route, _row_args), every public method with its docstring, and the thin pieces that choose between the HIP library
and the host (_order_cohort, _lattice_whole, _lattice_at).  What the methods return is in results.py.  The host
definitions every device kernel is tested against are methods MetMHN inherits: order_host.py has the order family
(tables, walks, Viterbi / Pareto, the sum-product passes and the quantities computed from them - the recurrence
described above is its _settle / _advance / _total), lattice_host.py the seeding forecast and the sweeps over all 2^n
genotypes.  Their names are imported below, so `from metmhn_amd.model import ...` finds every one of them.
"""
from __future__ import annotations

import warnings
from types import SimpleNamespace

import numpy as np

from .jx import kronvec as _kronvec
from .state import MetState, State
# re-exported, callers import them from here: the result containers (results.py), the host definitions MetMHN inherits
# and their helpers (order_host.py, lattice_host.py), and _philox, which sample_order's docstring names
from . import _philox  # noqa: F401
from .lattice_host import _FORECAST_HOST_MAX, _LATTICE_HOST_MAX, _LatticeHost  # noqa: F401
from .order_host import _OrderHost, _pareto, _single_diag, _subset_index, _subset_sums  # noqa: F401
from .results import (GENOTYPE_STRATA, METASTASIS_STRATA, PARTNER_STRATA, GenotypeDistribution,  # noqa: F401
                      GenotypeSummary, MetastasisDistribution, MetastasisSummary, OrderPosition, OrderPositions,
                      OrderPosterior, OrderPosteriors, OrderPrecedence, OrderPrecedences, OrderSample, OrderSamples,
                      OrderSnapshot, OrderSnapshots, OrderTime, OrderTimes, PartnerDistribution, PartnerSummary,
                      SeedingForecast, SeedingForecasts, SeedingLandscape, _entry_times)

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
_FORECAST_UNTIL = ("seeding", "observation")
_PARTNER_GIVEN = ("PT", "MT")
_NO_SEEDING_EXIT = ("the seeding rate of the full genotype underflows to 0 (a theta[n, n] of -1e10, as a fit without seeded "
                    "samples leaves it?): until='seeding' the full state would have no exit; use until='observation'")


def _check_backend(backend: str) -> None:
    if backend not in ("device", "host"):
        raise ValueError("backend must be 'device' or 'host'")


class MetMHN(_OrderHost, _LatticeHost):
    """The metastasis MHN with its two observation-rate vectors (model.py:175-211): the public surface and the choice
    between the HIP library and the host definitions, which it inherits (order_host.py, lattice_host.py)."""

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
        # <what>_fallback_rows: the rows the last likeliest_orders (orders), order_posteriors, order_precedences,
        # order_positions, order_times, order_snapshots or sample_orders (samples) call recomputed on the host
        for what in ("orders", "posteriors", "precedences", "positions", "times", "snapshots", "samples"):
            setattr(self, what + "_fallback_rows", 0)

    def _check_dat(self, dat) -> np.ndarray:
        """A reference-format cohort as an array [n_pat, 2n+3]."""
        dat = np.asarray(dat)
        if dat.ndim != 2 or dat.shape[1] != 2 * self.n + 3:
            raise ValueError(f"dat must have shape [n_pat, {2 * self.n + 3}]")
        return dat

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
        dat = self._check_dat(dat)
        _check_backend(backend)
        if backend == "host":
            self.orders_fallback_rows = 0
            return [self._row_order(dat, i) for i in range(dat.shape[0])]
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
        dat = self._check_dat(dat)
        _check_backend(backend)
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
        single = self._chain_tables(chain, st)
        return self._posterior_single(single[0]) if single else self._posterior_paired(st, first_obs)

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
        single = self._chain_tables(chain, st)
        return self._precedence_single(*single) if single else self._precedence_paired(st, first_obs)

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
        single = self._chain_tables(chain, st)
        if not single:
            return self._position_paired(st, first_obs)
        le, pos = self._position_single(single[0])
        nan = np.full((self.n + 1, self.n + 1), np.nan)
        return OrderPosition(le, nan, pos) if chain == "mt" else OrderPosition(le, pos, nan)

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
        single = self._chain_tables(chain, st)
        return self._time_single(*single) if single else self._time_paired(st, first_obs)

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
        single = self._chain_tables(chain, st)
        if not single:
            return self._snapshot_paired(st, first_obs)
        return self._snapshot_none(float(np.log(self._single_passes(single[0])[1])))

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
        single = self._chain_tables(chain, st)
        if not single:
            return self._sample_paired(st, first_obs, samples, key, row)
        return self._sample_single(*single, samples, key, row)

    def sample_orders(self, dat, n_samples: int, key: int = 0, first: int = 0, backend: str = "device") -> "OrderSamples":
        """sample_order of every row of a reference-format `dat` [n_pat, 2n+3], rows read as order_posteriors reads them,
        row i with row=i: arrays log_evidence [n_pat], orders [n_pat, n_samples, 2n+1] (int8), log_prob [n_pat, n_samples].

        backend="device": every row in one call of the HIP library (mmhn_order_samples); a row whose lattice and samples
        do not fit the workspace is drawn here with sample_order - how many were is left in `self.samples_fallback_rows`.
        backend="host": sample_order row by row.  An invalid row raises likeliest_order's ValueError, with its index."""
        dat = self._check_dat(dat)
        _check_backend(backend)
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

    def seeding_forecast(self, genotype, until: str = "seeding") -> "SeedingForecast":
        """The forward question: a primary tumour holds the mutations of `genotype` (n entries 0 / 1) and has not seeded -
        what happens until the seeding (until="seeding"), or until the seeding or the first observation on the model's own
        clock, whichever comes first (until="observation")?  See SeedingForecast for the answers.

        Exact: before the seeding the chain runs on the supersets y of the genotype, a lattice over the f mutations it does
        not hold, with rates lambda_j(y) = exp(theta_jj + sum_{i in y} theta_ji) (j not in y), sigma(y) the same for the
        seeding (the primary tumour's theta: theta[:n, n] is not read) and kappa(y) = exp(sum_{i in y} obs1_i) for the clock
        (0 until the seeding); den = sum lambda + sigma + kappa.  F(genotype) = 1, F(y) = sum_b F(y - b) lambda_b(y - b) /
        den(y - b) is the probability of reaching y, G = F / den the expected time spent there, and every answer is a sum of
        G times a rate.  This is the host definition (lattice_host.py: _forecast_host), level by level in NumPy (f <= 24);
        seeding_forecasts has the device."""
        g = self._forecast_checks(np.asarray(genotype)[None, :] if np.ndim(genotype) == 1 else genotype, until)
        if g.shape[0] != 1:
            raise ValueError("seeding_forecast takes one genotype; seeding_forecasts takes many")
        return self._forecast_host(g[0], until)

    def seeding_forecasts(self, genotypes, until: str = "seeding", backend: str = "device") -> "SeedingForecasts":
        """seeding_forecast of every row of `genotypes` [R, n] (of a cohort `dat`: dat[:, 0:2*n:2], the primary tumours'
        columns): arrays p_seed [R], time [R], before [R, n], with_seed [R, n], n_before [R, n+1], next [R, n+1].
        Identical genotypes are solved once.

        backend="device": every distinct genotype in one call of the HIP library (mmhn_seeding_forecasts), a lattice of
        8 B x 2^f per row spread over the whole GPU, level by level.  A row that does not fit (more than 30 free mutations,
        or a lattice larger than the workspace limit) raises a ValueError that names the row and the bytes it needs: there
        is no host fallback, a host lattice of 2^28 states is none.  backend="host": seeding_forecast row by row.
        An entry other than 0 / 1 raises ValueError("row i: ...")."""
        _check_backend(backend)
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
        _check_backend(backend)
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
        _check_backend(backend)
        return self._lattice_at(genotypes, until, backend, 4, lambda: self._landscape_host(until),
                                self._landscape_device(until), SeedingLandscape)

    # ------------------------------------------------------------------ genotype distribution of the primary tumour
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
        _check_backend(backend)
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
        _check_backend(backend)
        return self._lattice_at(genotypes, "observation", backend, 2, self._genodist_host, self._genodist_device,
                                GenotypeDistribution, self._genodist_summary_host, GenotypeSummary)

    # ------------------------------------------------------------------ genotype distribution of the metastasis and its founder
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
        _check_backend(backend)
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
        _check_backend(backend)
        return self._lattice_at(genotypes, "observation", backend, 3, self._metdist_host, self._metdist_device,
                                MetastasisDistribution, self._metdist_summary_host, MetastasisSummary)

    # ------------------------------------------------------------------ genotype distribution of one tumour given the other
    def _lattice_max_bytes(self, max_bytes, planes, noun, prep, at):
        """_lattice_whole's refusal of a result of `planes` values per genotype that exceeds max_bytes."""
        n = self.n
        if 8 * planes << n > max_bytes:
            raise ValueError(f"{n} mutations: a {noun} {prep} 2^{n} genotypes needs {8 * planes << n} bytes, more than max_bytes = "
                             f"{int(max_bytes)}; {at} reads single genotypes off the device's {noun}")

    def _partner_checks(self, given, backend):
        if given not in _PARTNER_GIVEN:
            raise ValueError("given must be 'PT' or 'MT'")
        _check_backend(backend)

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

    # ------------------------------------------------------------------ second moments of the (PT x MT) table
    def cross_distribution(self, backend: str = "device", burden: bool = True) -> "CrossSummary":
        """The exact PT x MT co-occurrence and joint burden tables of a seeded pair - the second moments of the table of which
        partner_distribution gives one row or column: cross[i, j] = P(PT holds i, MT holds j, seeded), burden[k, l] =
        P(|PT| = k, |MT| = l, seeded), with the marginals pt, mt, the mixed gene_burden and mass = P(seeded) (CrossSummary;
        everything joint with "seeded").  After the seeding the two tumours are independent chains, so every bilinear
        statistic of the pair factorises through the founder z.  With partner_distribution's symbols and Z = sigma G0,
        metastasis_distribution's founder:
            a_phi(z) = (kappa1(z) phi(z) + sum_{j not in z} lambda_j(z) a_phi(z + j)) / den1(z)     from the full genotype down
            b_psi(z) the same with mu, kappam, denm;        E[phi(PT) psi(MT); seeded] = sum_z Z(z) a_phi(z) b_psi(z)
        phi = [mutation i held] gives `cross`, phi = [|x| = k] gives `burden`.  The full (PT x MT) table has no such form: it
        needs the 2^(2n+1) joint space; its second moments do not.

        backend="device": one call of the HIP library (mmhn_cross_table): 2 ceil((2n+1)/4) backward sweeps of four planes
        when 8 B x 2^n x (5 + 4 ceil((2n+1)/4)) fit the workspace limit, more sweeps and the same bytes when only fewer
        planes fit (72 B x 2^n at the least); nothing of size 2^n comes back.  burden=False sweeps the n gene features only:
        burden and gene_burden are NaN, the rest has the same bytes.  backend="host": the definition in NumPy
        (lattice_host.py: _cross_host), n <= 24, always with the burden.  (CrossSummary and PairedSummary live in
        metmhn_amd.results; this module's public names are pinned.)"""
        from .results import CrossSummary
        _check_backend(backend)
        n = self.n
        if backend == "host":
            c = self._cross_host()
            got = (c.mass, c.pt, c.mt, c.cross, c.burden, c.gene_burden)
            if not burden:
                got = got[:4] + (np.full((n + 1, n + 1), np.nan), np.full((2, n, n + 1), np.nan))
        else:
            from .jx import engine
            got = engine(n).cross_table(self.log_theta, self.obs1, self.obs2, burden=bool(burden))
        return CrossSummary(*got)

    def paired_summary(self, backend: str = "device") -> "PairedSummary":
        """The exact pairwise frequencies of a seeded pair over the columns [PT_0, MT_0, PT_1, MT_1, ...] - the exact form of
        simulate_pairs(...).frequencies("paired") and, through compare(dat), of the posterior-predictive check of a cohort's
        paired rows: cross_distribution for the PT x MT block and the two one-tumour sweeps for the others
        (genotype_distribution_at's and metastasis_distribution_at's summaries; no plane comes back)."""
        from .results import PairedSummary
        _check_backend(backend)
        none = np.zeros((0, self.n), dtype=np.int8)
        return PairedSummary(self.genotype_distribution_at(none, backend).summary,
                             self.metastasis_distribution_at(none, backend).summary, self.cross_distribution(backend))
