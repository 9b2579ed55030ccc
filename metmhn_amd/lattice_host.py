"""Host definitions of the seeding forecast and of the five sweeps over all 2^n genotypes: what the device kernels of
csrc/forecast.h, landscape.h, genodist.h, metdist.h, partner.h and cross.h are tested against and what their comments send the
reader to.  NumPy, level by level over the popcount of the genotype code, the moves of a level in the order of their
bit - the order the kernels are checked against, so nothing here is reordered or fused.

What it holds, top to bottom.  _level_moves, the ascending level sweep that the forecast, the two distributions and both
sweeps of _partner_host share.  Then class _LatticeHost, which model.MetMHN inherits: the rates (_lattice_host_rates:
lambda and sigma; _lattice_host_chains: with them the metastasis' rates, the three clocks and the three denominators),
_forecast_next and _forecast_host (seeding_forecast behind its checks), _landscape_host (the one descending sweep, four
numerators per move: it shares the rates only), _genodist_host, _metdist_host, _partner_rates and _partner_host, the
three summaries by their definition (_genodist_summary_host, _metdist_summary_host, _partner_summary_host), and _cross_host
(the founder plane by _metdist_host's lines, a descending sweep per chain over all features, the fold).

Who calls it.  MetMHN's forecast and lattice entry points (model.py) for backend="host": seeding_forecast always, the
others through _lattice_whole / _lattice_at, which choose between these and the HIP library.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from .order_host import _subset_sums
from .results import GenotypeSummary, MetastasisSummary, PartnerSummary, SeedingForecast

_FORECAST_HOST_MAX = 24          # free mutations the host definition takes on: f x 2^f doubles of rates
_LATTICE_HOST_MAX = 24           # mutations the host landscape and distributions take on: n x 2^n doubles of rates


def _level_moves(levels, bits: int, planes):
    """The ascending level sweep: for every level's states ys (`levels`, lowest first) the moves into it, bit by bit -
    F[y] += G[y - b] rate[b][y - b] for every plane (F, G, rate) - and then the level is handed to the caller as (lev, ys)
    to form G[ys] from F[ys], the step that couples planes included, before the next level reads it."""
    for lev, ys in enumerate(levels):
        for b in range(bits if lev else 0):
            to = ys[(ys >> b & 1) == 1]
            frm = to ^ (1 << b)
            for F, G, rate in planes:
                F[to] += G[frm] * rate[b][frm]
        yield lev, ys


class _LatticeHost:
    """The host definitions of the forecast and the lattice sweeps as methods of MetMHN (model.MetMHN inherits them).
    They read the model through self: log_theta, _pt_log_theta, obs1, obs2, n."""

    # ------------------------------------------------------------------ rates
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

    def _lattice_host_chains(self):
        """_lattice_host_rates of the distributions with what their three chains add: mu [n], the metastasis' rates; the
        clocks kap0 (primary tumour, unseeded), kap1 (seeded) and kapm (metastasis); and the denominators den0 = L + sig +
        kap0, den1 = L + kap1 and denm = Lm + kapm, L and Lm the summed lam and mu of the mutations a genotype lacks."""
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
        return SimpleNamespace(idx=idx, level=level, lam=lam, mu=mu, sig=sig, kap0=kap0, kap1=kap1, kapm=kapm,
                               den0=L + sig + kap0, den1=L + kap1, denm=Lm + kapm)

    # ------------------------------------------------------------------ seeding forecast
    def _forecast_next(self, g: np.ndarray, until: str) -> np.ndarray:
        """next [R, n+1] of the genotypes g [R, n]: the rates out of the genotype over their sum with the clock."""
        th, n = self._pt_log_theta, self.n
        rate = np.exp(np.diag(th)[None, :] + g @ th[:, :n].T)                      # [R, n+1]: lambda_j(x), sigma(x)
        rate[:, :n] = np.where(g == 1, 0.0, rate[:, :n])
        kap = np.exp(g @ self.obs1[:n]) if until == "observation" else 0.0
        out = rate / (rate.sum(axis=1) + kap)[:, None]
        out[:, :n] = np.where(g == 1, np.nan, out[:, :n])
        return out

    def _forecast_host(self, g: np.ndarray, until: str) -> "SeedingForecast":
        """seeding_forecast of the checked genotype g [n] (its docstring has the recurrence): the lattice over the f
        mutations g does not hold, level by level."""
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
        for _, ys in _level_moves((idx[level == lev] for lev in range(f + 1)), f, ((F, G, lam),)):
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

    # ------------------------------------------------------------------ genotype distribution of the primary tumour
    def _genodist_host(self) -> np.ndarray:
        """[2, 2^n]: the definition of the genotype distribution (U, S), level by level over the popcount, ascending."""
        n, size = self.n, 1 << self.n
        R = self._lattice_host_chains()
        F0, F1, G0, G1 = (np.zeros(size) for _ in range(4))
        F0[0] = 1.0
        levels = (R.idx[R.level == lev] for lev in range(n + 1))
        for _, ys in _level_moves(levels, n, ((F0, G0, R.lam), (F1, G1, R.lam))):
            G0[ys] = F0[ys] / R.den0[ys]
            F1[ys] = G0[ys] * R.sig[ys] + F1[ys]
            G1[ys] = F1[ys] / R.den1[ys]
        return np.stack((R.kap0 * G0, R.kap1 * G1))

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

    # ------------------------------------------------------------------ genotype distribution of the metastasis and its founder
    def _metdist_host(self) -> np.ndarray:
        """[3, 2^n]: the definition of the metastasis distribution (Z, M, C), level by level over the popcount, ascending."""
        n, size = self.n, 1 << self.n
        R = self._lattice_host_chains()
        F0, FM, FC, G0, GM, GC = (np.zeros(size) for _ in range(6))
        F0[0] = 1.0
        levels = (R.idx[R.level == lev] for lev in range(n + 1))
        for lev, ys in _level_moves(levels, n, ((F0, G0, R.lam), (FM, GM, R.mu), (FC, GC, R.mu))):
            G0[ys] = F0[ys] / R.den0[ys]
            seeded = G0[ys] * R.sig[ys]
            FM[ys] = seeded + FM[ys]
            FC[ys] = seeded * lev + FC[ys]
            GM[ys] = FM[ys] / R.denm[ys]
            GC[ys] = FC[ys] / R.denm[ys]
        return np.stack((R.sig * G0, R.kapm * GM, R.kapm * GC))

    @staticmethod
    def _metdist_summary_host(P: np.ndarray) -> "MetastasisSummary":
        """The MetastasisSummary of the planes P [3, 2^n] (Z and M are summed), by its definition."""
        s = _LatticeHost._genodist_summary_host(P[:2])
        return MetastasisSummary(s.mass, s.pairs, s.burden)

    # ------------------------------------------------------------------ genotype distribution of one tumour given the other
    def _partner_rates(self):
        """What _partner_host needs of the model, formed once for any number of queries."""
        R = self._lattice_host_chains()
        chains = {"PT": (R.lam, R.kap1, R.den1), "MT": (R.mu, R.kapm, R.denm)}
        return R.idx, R.level, R.lam, R.sig, R.den0, chains

    def _partner_host(self, q: int, given: str, rates=None) -> np.ndarray:
        """[2, 2^n]: the definition of the partner distribution (W, J) of the query code q, level by level."""
        n, size = self.n, 1 << self.n
        idx, level, lam, sig, den0, chains = rates if rates is not None else self._partner_rates()
        (rq, kq, dq), (rp, kp, dp) = chains[given], chains["MT" if given == "PT" else "PT"]
        sub = (idx & ~q) == 0
        top = bin(q).count("1")
        F0, G0, B = (np.zeros(size) for _ in range(3))
        F0[0] = 1.0
        levels = (idx[(level == lev) & sub] for lev in range(top + 1))
        for _, ys in _level_moves(levels, n, ((F0, G0, lam),)):      # G0 on the subsets of q
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
        levels = (idx[level == lev] for lev in range(n + 1))
        for _, ys in _level_moves(levels, n, ((F, G, rp),)):         # the partner's chain from every founder at once
            G[ys] = F[ys] / dp[ys]
        return np.stack((W, kp * G))

    @staticmethod
    def _partner_summary_host(P: np.ndarray) -> "PartnerSummary":
        """The PartnerSummary of the planes P [2, 2^n], by its definition."""
        s = _LatticeHost._genodist_summary_host(P)
        return PartnerSummary(s.mass, s.pairs, s.burden)

    # ------------------------------------------------------------------ second moments of the (PT x MT) table
    def _cross_host(self, planes: bool = False):
        """The definition of the cross table: mass, pt [n], mt [n], cross [n, n], burden [n+1, n+1], gene_burden
        [2, n, n+1], all joint with "seeded".  After the seeding the two tumours are independent chains, so a bilinear
        statistic of the pair factorises through the founder z: E[phi(PT) psi(MT); seeded] = sum_z Z(z) a_phi(z) b_psi(z)
        with Z = sigma G0 (_metdist_host's founder plane, the same lines) and the value functions
            a_phi(z) = (kappa1(z) phi(z) + sum_{j not in z} lambda_j(z) a_phi(z + j)) / den1(z)
        of the primary tumour's chain, b_psi the same with mu, kappam, denm - level by level over the popcount, descending,
        the moves of a state in ascending bit.  The 2 n + 1 features of a chain: the n gene indicators, then the n + 1
        burden indicators.  With `planes` also Z [2^n] and the value functions A, B [2 n + 1, 2^n]."""
        n, size = self.n, 1 << self.n
        R = self._lattice_host_chains()
        F0, G0 = np.zeros(size), np.zeros(size)
        F0[0] = 1.0
        levels = (R.idx[R.level == lev] for lev in range(n + 1))
        for _, ys in _level_moves(levels, n, ((F0, G0, R.lam),)):
            G0[ys] = F0[ys] / R.den0[ys]
        Z = R.sig * G0
        phi = np.stack([(R.idx >> i & 1).astype(np.float64) for i in range(n)] +
                       [(R.level == k).astype(np.float64) for k in range(n + 1)])
        values = []
        for rate, kap, den in ((R.lam, R.kap1, R.den1), (R.mu, R.kapm, R.denm)):
            a = np.zeros((2 * n + 1, size))
            for lev in range(n, -1, -1):
                xs = R.idx[R.level == lev]
                num = np.zeros((2 * n + 1, len(xs)))
                for j in range(n):
                    m = (xs >> j & 1) == 0
                    x = xs[m]
                    num[:, m] += rate[j][x] * a[:, x | 1 << j]
                a[:, xs] = (kap[xs] * phi[:, xs] + num) / den[xs]
            values.append(a)
        A, B = values
        M = np.stack([((Z * a) * B).sum(axis=1) for a in A])      # [f, g] = sum_z (Z a_f) b_g, NumPy's pairwise sums
        out = SimpleNamespace(mass=float(Z.sum()), pt=(Z * A[:n]).sum(axis=1), mt=(Z * B[:n]).sum(axis=1),
                              cross=np.ascontiguousarray(M[:n, :n]), burden=np.ascontiguousarray(M[n:, n:]),
                              gene_burden=np.stack((M[:n, n:], M[n:, :n].T)))
        if planes:
            out.Z, out.A, out.B = Z, A, B
        return out
