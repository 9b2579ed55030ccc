"""Host definitions of the order family: what the device kernels of csrc/order*.h are tested against and what their
comments send the reader to.  One observation at a time, plain Python / NumPy loops over the 2^k sub-states of its k
occupied slots, in the loop order the kernels follow - nothing here is vectorised on purpose.

What it holds, top to bottom.  The lattice helpers (_subset_sums, _subset_index, _single_diag, _pareto).  Then class
_OrderHost, which model.MetMHN inherits: the tables of a one-tumour chain (_single_tables; _chain_tables picks the chain
_route named) with its walk, Viterbi pass, forward pass (_single_forward) and the two sum-product passes
(_single_passes) and the quantities computed from them (_posterior_single ... _sample_single); then the same for a
paired row - _paired_tables, the prefix-vector recurrence (_settle, _advance, _total; model.py's docstring explains the
vector), _likelihood_paired, _paired_passes, _unseeded_backward, _paired_moves and _posterior_paired ...
_sample_paired, _likeliest_order_paired.

Who calls it.  MetMHN's one-observation entry points (model.py: likelihood, likeliest_order, order_posterior,
order_precedence, order_position, order_time, order_snapshot, sample_order) route an observation and call the
_*_single / _*_paired method of its chain; the cohort wrappers call those for backend="host" and for the rows the device
turned away.  The one device call is MetMHN._get_diag_paired (model.py), reached through self from _paired_tables.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import _philox
from .results import OrderPosition, OrderPosterior, OrderPrecedence, OrderSample, OrderSnapshot, OrderTime
from .state import MetState, State


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


class _OrderHost:
    """The host definitions of the order family as methods of MetMHN (model.MetMHN inherits them).  They read the model
    through self - log_theta, _pt_log_theta, obs1, obs2, n - and reach one another and MetMHN's two diagonals through
    self as well, so an instance can have any of them replaced."""

    # ------------------------------------------------------------------ one tumour
    def _chain_tables(self, chain: str, st):
        """The one-tumour chain `_route` named for an observation: its tables and the event codes of their slots - "mt":
        the metastasis under log_theta and obs2, codes 2e+1 and 2n for the seeding; "pt": the primary tumour under
        _pt_log_theta and obs1, codes 2e.  None for "paired", which has tables of its own (_paired_tables)."""
        if chain == "mt":
            T = self._single_tables(self.log_theta, st, self.obs2)
            return T, [2 * self.n if e == self.n else 2 * e + 1 for e in T.ev]
        if chain == "pt":
            T = self._single_tables(self._pt_log_theta, st, self.obs1)
            return T, [2 * e for e in T.ev]
        return None

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

    @staticmethod
    def _single_forward(T):
        """_single_viterbi's recurrence with the maximum replaced by the sum: F[x] = the summed probability of the
        prefixes that lead to x (1 / den[x] included), and the evidence Z."""
        k, V = T.k, 1 << T.k
        F = np.zeros(V)
        F[0] = 1.0 / T.den[0]
        for x in range(1, V):
            s = 0.0
            for b in range(k):
                if x >> b & 1:
                    s += F[x ^ 1 << b] * T.num[b][x]
            F[x] = s / T.den[x]
        return F, F[-1] * T.final

    def _posterior_single(self, T) -> "OrderPosterior":
        """_single_forward, and the transpose of its recurrence over the seeded half."""
        n, k, V = self.n, T.k, 1 << T.k
        F, Z = self._single_forward(T)
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
        """_single_forward's F and evidence Z, and the backward pass over the whole lattice as G[x] = B[x] / den[x]: the
        move x -> y = x | d has the mass F[x] num_d[y] G[y]."""
        k, V = T.k, 1 << T.k
        F, Z = _OrderHost._single_forward(T)
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
        return self._single_walk(self._chain_tables("mt", State(events, size=self.n + 1))[0], events)

    def _likeliest_order_unpaired_mt(self, state: State):
        """model.py:448-501."""
        events, p = self._single_viterbi(self._chain_tables("mt", state)[0])
        codes = 2 * events + 1
        codes[events == self.n] = 2 * self.n
        return codes, p

    def _likelihood_unpaired_pt(self, order) -> float:
        """model.py:343,356: the reference hands these to mhn.oMHN(vstack(theta with the seeding's
        column zeroed, obs1)).order_likelihood -- a one-tumour chain over the n+1 events whose
        observation rate is exp(obs1 . state); expansion in the reference's tests/test_orders.py:76-100."""
        events = [e // 2 for e in order]
        return self._single_walk(self._chain_tables("pt", State(events, size=self.n + 1))[0], events)

    def _likeliest_order_unpaired_pt(self, state: State):
        """model.py:260-274 (mhn.oMHN.likeliest_order on the same chain)."""
        events, p = self._single_viterbi(self._chain_tables("pt", state)[0])
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
        a, bp, bm = _OrderHost._settle(T, x, v)
        num = T.num[b][y]
        bp = bp * num / T.den_mt[y] if T.pt_first and T.kind[b] == 1 else 0.0
        bm = bm * num / T.den_pt[y] if T.mt_first and T.kind[b] == 0 else 0.0
        return y, (a * num / T.den[y], bp, bm)

    @staticmethod
    def _total(T, v) -> float:
        full = (1 << T.k) - 1
        a, bp, bm = _OrderHost._settle(T, full, v)
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

    def _paired_moves(self, T, F, B, Bu):
        """Every move of a paired row with its mass, (state x, slots it adds, w), x over F in insertion order: from a
        seeded x the slots d it lacks, ascending, w = B[x | d] . A(x, d) F[x]; from an unseeded x the seeding edge, then
        the joint moves ascending (slots b and b + 1), w = F[x]_a A(x, b) Bu[x | b | b + 1]."""
        k = T.k
        top = 1 << (k - 1)
        for x in F:
            if x & top:
                for d in range(k - 1):
                    if not x >> d & 1:
                        y, v = self._advance(T, x, F[x], d)
                        g = B[y]
                        yield x, (d,), g[0] * v[0] + g[1] * v[1] + g[2] * v[2]
                continue
            y = x | top
            yield x, (k - 1,), B[y][0] * (F[x][0] * T.num[k - 1][y] / T.den[y])
            for b in range(k - 1):
                if T.joint >> b & 1 and not x >> b & 1:
                    y = x | 3 << b
                    yield x, (b, b + 1), F[x][0] * T.num[b][y] / T.den[y] * Bu[y]

    def _position_paired(self, state: MetState, first_obs: str) -> "OrderPosition":
        """_paired_moves' masses, added to the position popcount(x & the slots of the lineage) of the event the move adds,
        in every lineage that has the slot: the seeding is in both, and before it both tumours agree, so a state of j
        joint events puts the move's event at j in both lineages."""
        T, F, Z, B = self._paired_passes(state, first_obs)
        n, k = self.n, T.k
        top = 1 << (k - 1)
        ev = [n if s == 2 * n else s // 2 for s in T.slots]
        count = lambda x: bin(x).count("1")
        pos_pt, pos_mt = np.full((n + 1, n + 1), np.nan), np.full((n + 1, n + 1), np.nan)
        for d in range(k):
            if T.kind[d] != 1:
                pos_pt[ev[d]] = 0.0
            if T.kind[d] != 0:
                pos_mt[ev[d]] = 0.0
        for x, added, w in self._paired_moves(T, F, B, self._unseeded_backward(T, F, B)):
            for d in added:
                if T.kind[d] != 1:
                    pos_pt[ev[d], count(x & (T.pt_mask | top))] += w
                if T.kind[d] != 0:
                    pos_mt[ev[d], count(x & (T.mt_mask | top))] += w
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
        joint moves and the seeding edge), and the mass of EVERY move (_paired_moves) added to P[c, d] for the slots c its
        state holds and the slot(s) d it adds - a joint move adds both of its slots, so neither precedes the other."""
        T, F, Z, B = self._paired_passes(state, first_obs)
        k = T.k
        P = np.zeros((k, k))
        for x, added, w in self._paired_moves(T, F, B, self._unseeded_backward(T, F, B)):
            for c in range(k):
                if x >> c & 1:
                    for d in added:
                        P[c, d] += w
        return OrderPrecedence(float(np.log(Z)), self._precedence_matrix(T.slots, P, Z))

    def _sample_paired(self, state: MetState, first_obs: str, samples, key, row) -> "OrderSample":
        """sample_order on a paired row: _unseeded_backward's terms before the seeding, then the three terms of a seeded
        move's mass (_paired_moves) with the path's own prefix vector in F's place."""
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
