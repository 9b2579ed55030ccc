"""Python handle on the native engine (one engine = one GPU)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import f64p, i8p, i64p

F64, F32 = 0, 1
_DEFAULT = {"device": None}


def set_default_device(device: int | None):
    """GPU used by every Engine created without an explicit `device` (jx mirrors, simulations, the objective).
    None: LOCAL_RANK of a torch.distributed launch, else 0."""
    _DEFAULT["device"] = None if device is None else int(device)


def default_device() -> int:
    if _DEFAULT["device"] is not None:
        return _DEFAULT["device"]
    import os
    return int(os.environ.get("LOCAL_RANK", "0"))


def unique_id() -> bytes:
    """128-byte RCCL id for Engine.comm_init (call on one rank, hand to the others by any host channel)."""
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mmhn_comm_unique_id(buf))
    return buf.raw


def _f(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(f64p)


def _s(a):
    a = np.ascontiguousarray(np.asarray(a).astype(np.int8))
    return a, a.ctypes.data_as(i8p)


def _vec(a, V, name):
    """float64 copy of a vector of length V (a restricted state vector, V = 2^k)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.shape != (V,):
        raise ValueError(f"{name} must have shape ({V},), got {a.shape}")
    return a, a.ctypes.data_as(f64p)


class Engine:
    """Owns a mmhn_handle.  `n_mut` mutations -> N = n_mut + 1 events incl. seeding."""

    def __init__(self, n_mut: int, device: int | None = None, dtype: str = "f64", workspace_bytes: int | None = None):
        self.lib = _lib.load()
        if device is None:
            device = default_device()
        self.device = int(device)
        self.n = int(n_mut)
        self.N = self.n + 1
        self.dtype = dtype
        h = C.c_void_p()
        _lib.check(self.lib.mmhn_create(int(device), self.n, F64 if dtype == "f64" else F32, C.byref(h)))
        self.h = h
        self.n_pat = 0
        self._row_weights = None
        self._row_groups = None
        self.comm_size = 1
        if workspace_bytes:
            _lib.check(self.lib.mmhn_set_workspace_limit(self.h, int(workspace_bytes)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        if getattr(self, "h", None):
            self.lib.mmhn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- cohort objective
    def set_cohort(self, dat):
        dat = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
        if dat.ndim != 2 or dat.shape[1] != 2 * self.n + 3:
            raise ValueError(f"dat must be [n_pat, {2 * self.n + 3}]")
        try:
            _lib.check(self.lib.mmhn_set_cohort(self.h, dat.ctypes.data_as(i8p), dat.shape[0], dat.shape[1]))
        except RuntimeError as err:
            # a cohort that the library refused or could not place leaves it without one; a call turned away while an
            # evaluation is pending never read the rows, and the library keeps the cohort it has
            if "has not been collected" not in str(err):
                self.n_pat = 0
                self._row_weights = None
                self._row_groups = None
            raise
        self.n_pat = dat.shape[0]
        self._row_weights = None                              # (mmhn_set_cohort clears them)
        self._row_groups = None

    def set_row_weights(self, w):
        """One weight per row of the current cohort (mmhn_set_row_weights): w_i >= 0, finite, not all zero; None removes
        them.  Every cohort sum becomes the weighted sum of the per-row values, the counts the weighted counts
        (`row_weight_sums`); for integer weights that is the objective of the cohort with row i written w_i times.  A row of
        weight 0 counts as absent (it is still solved).  patient_grads / patient_status stay per row and unweighted.  The
        weights go to the device here, once; set_cohort clears them."""
        if w is None:
            _lib.check(self.lib.mmhn_set_row_weights(self.h, None, 0))
            self._row_weights = None
            return
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
        if w.ndim != 1:
            raise ValueError(f"weights must have shape ({self.n_pat},), got {w.shape}")
        if self.n_pat > 0 and w.shape[0] != self.n_pat:
            raise ValueError(f"weights must have shape ({self.n_pat},), got {w.shape}: one weight per cohort row "
                             f"(row {min(w.shape[0], self.n_pat)} has no counterpart)")
        _lib.check(self.lib.mmhn_set_row_weights(self.h, w.ctypes.data_as(f64p), w.shape[0]))
        self._row_weights = w.copy()

    @property
    def row_weights(self):
        """A copy of the weights the engine holds, or None."""
        w = getattr(self, "_row_weights", None)
        return None if w is None else w.copy()

    @property
    def row_weight_sums(self):
        """(n_em, n_pat, n_unknown) of this engine's rows: the weighted sums with weights set, else the integer counts."""
        out = np.zeros(3)
        _lib.check(self.lib.mmhn_get_row_weight_sums(self.h, out.ctypes.data_as(f64p)))
        return float(out[0]), float(out[1]), float(out[2])

    def set_row_groups(self, ptr, rows, w=None):
        """Row groups of the current cohort (mmhn_set_row_groups): group g is the list rows[ptr[g]:ptr[g+1]] of cohort rows -
        the alternatives of one patient, e.g. the completions of a row with unobserved entries - with the weight w[g] >= 0
        (default: ones).  The group's likelihood is the sum of its rows': lp_g = logsumexp(lp_r), and every gradient sum takes
        row r with rho = exp(lp_r - lp_g); the counts (`row_weight_sums`) are the group-weighted ones.  A row in no group, or
        only in groups of weight 0, counts as absent (it is still solved).  patient_grads / patient_status stay per row and
        unmixed.  ptr=None removes the groups; set_cohort clears them.  Row weights and row groups exclude each other, and
        groups need a one-rank engine."""
        if ptr is None:
            _lib.check(self.lib.mmhn_set_row_groups(self.h, None, 0, None, None))
            self._row_groups = None
            return
        ptr = np.ascontiguousarray(np.asarray(ptr, dtype=np.int64))
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        if ptr.ndim != 1 or rows.ndim != 1 or ptr.shape[0] < 1:
            raise ValueError(f"ptr must have shape (n_groups + 1,) and rows (ptr[-1],), got {ptr.shape} and {rows.shape}")
        ng = ptr.shape[0] - 1
        w = np.ones(ng) if w is None else np.ascontiguousarray(np.asarray(w, dtype=np.float64))
        if w.shape != (ng,):
            raise ValueError(f"w must have shape ({ng},): one weight per group, got {w.shape}")
        if ng > 0 and not (0 <= ptr[-1] <= rows.shape[0] and (ptr <= rows.shape[0]).all() and (ptr >= 0).all()):
            bad = int(np.argmax((ptr > rows.shape[0]) | (ptr < 0)))
            raise ValueError(f"ptr[{bad}] = {int(ptr[bad])} points outside rows (length {rows.shape[0]}): group {max(bad - 1, 0)}")
        if ng == 0:
            _lib.check(self.lib.mmhn_set_row_groups(self.h, None, 0, None, None))
            self._row_groups = None
            return
        _lib.check(self.lib.mmhn_set_row_groups(self.h, ptr.ctypes.data_as(i64p), ng, rows.ctypes.data_as(i64p),
                                                w.ctypes.data_as(f64p)))
        self._row_groups = (ptr.copy(), rows[:int(ptr[-1])].copy(), w.copy())

    @property
    def row_groups(self):
        """Copies of (ptr, rows, w) of the groups the engine holds, or None."""
        g = getattr(self, "_row_groups", None)
        return None if g is None else tuple(a.copy() for a in g)

    def group_posteriors(self, log_theta, log_d_p, log_d_m):
        """Score-only evaluation with row groups set (mmhn_group_posteriors): (lp_group [n_groups], rho [ptr[-1]]) with
        rho[ptr[g] + s] = P(the s-th alternative of group g | the group) = exp(lp_r - lp_g)."""
        if self._row_groups is None:
            raise RuntimeError("metmhn_amd: group_posteriors needs row groups (set_row_groups)")
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        ptr = self._row_groups[0]
        lpg, rho = np.zeros(ptr.shape[0] - 1), np.zeros(int(ptr[-1]))
        _lib.check(self.lib.mmhn_group_posteriors(self.h, a, b, c, lpg.ctypes.data_as(f64p), rho.ctypes.data_as(f64p)))
        return lpg, rho

    def _params(self, log_theta, log_d_p, log_d_m):
        lt, ltp = _f(log_theta)
        dp, dpp = _f(log_d_p)
        dm, dmp = _f(log_d_m)
        if lt.shape != (self.N, self.N) or dp.shape != (self.N,) or dm.shape != (self.N,):
            raise ValueError("parameter shapes do not match n_mut")
        return (lt, dp, dm), (ltp, dpp, dmp)

    def score(self, log_theta, log_d_p, log_d_m, perc_met):
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        out = C.c_double()
        _lib.check(self.lib.mmhn_score(self.h, a, b, c, float(perc_met), C.byref(out)))
        return out.value

    def score_and_grad(self, log_theta, log_d_p, log_d_m, perc_met):
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        out = C.c_double()
        g = np.zeros((self.N, self.N))
        gp = np.zeros(self.N)
        gm = np.zeros(self.N)
        _lib.check(self.lib.mmhn_score_and_grad(self.h, a, b, c, float(perc_met), C.byref(out),
                                                 g.ctypes.data_as(f64p), gp.ctypes.data_as(f64p),
                                                 gm.ctypes.data_as(f64p)))
        return out.value, g, gp, gm

    def cohort_sums(self, log_theta, log_d_p, log_d_m, with_grad=True):
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        sums = np.zeros(4 + 2 * self.N * self.N + 3 * self.N)
        _lib.check(self.lib.mmhn_cohort_sums(self.h, a, b, c, int(bool(with_grad)), sums.ctypes.data_as(f64p)))
        return sums

    def cohort_sums_begin(self, log_theta, log_d_p, log_d_m, with_grad=True):
        """Issue the evaluation and return at once (mmhn_cohort_sums_begin); collect with cohort_sums_end()."""
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        _lib.check(self.lib.mmhn_cohort_sums_begin(self.h, a, b, c, int(bool(with_grad))))

    def cohort_sums_end(self):
        sums = np.zeros(4 + 2 * self.N * self.N + 3 * self.N)
        _lib.check(self.lib.mmhn_cohort_sums_end(self.h, sums.ctypes.data_as(f64p)))
        return sums

    def cohort_wsums_begin(self, log_theta, log_d_p, log_d_m, w, with_grad=True, flag=None):
        """Like cohort_sums_begin with the EM / NM weighting applied on the device (mmhn_cohort_wsums_begin).
        flag (optional): one more double that rides in the same all-reduce (mmhn_set_reduce_flag); its sum over the ranks is
        `reduce_flag` after cohort_wsums_end."""
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        if flag is not None:
            _lib.check(self.lib.mmhn_set_reduce_flag(self.h, float(flag)))
        _lib.check(self.lib.mmhn_cohort_wsums_begin(self.h, a, b, c, int(bool(with_grad)), float(w)))

    def cohort_wsums_end(self):
        ws = np.zeros(1 + self.N * self.N + 2 * self.N)
        _lib.check(self.lib.mmhn_cohort_wsums_end(self.h, ws.ctypes.data_as(f64p)))
        out = C.c_double()
        _lib.check(self.lib.mmhn_get_reduce_flag(self.h, C.byref(out)))
        self.reduce_flag = out.value
        return ws

    def patient_grads(self, log_theta, log_d_p, log_d_m, with_grad=True):
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        P, N = self.n_pat, self.N
        lp = np.zeros(P)
        if not with_grad:
            _lib.check(self.lib.mmhn_patient_grads(self.h, a, b, c, lp.ctypes.data_as(f64p), None, None, None))
            return lp
        g, gp, gm = np.zeros((P, N, N)), np.zeros((P, N)), np.zeros((P, N))
        _lib.check(self.lib.mmhn_patient_grads(self.h, a, b, c, lp.ctypes.data_as(f64p), g.ctypes.data_as(f64p),
                                               gp.ctypes.data_as(f64p), gm.ctypes.data_as(f64p)))
        return lp, g, gp, gm

    def patient_status(self, log_theta, log_d_p, log_d_m):
        """Score-only evaluation of the current cohort (mmhn_patient_status): lp [n_pat] of every row and p_seeded [n_pat],
        P(the metastasis had been seeded | PT genotype) for the rows of type 4 (primary tumour, status unknown), NaN for
        every other row."""
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        lp, ps = np.zeros(self.n_pat), np.full(self.n_pat, np.nan)
        _lib.check(self.lib.mmhn_patient_status(self.h, a, b, c, lp.ctypes.data_as(f64p), ps.ctypes.data_as(f64p)))
        return lp, ps

    @property
    def n_unknown(self) -> int:
        """Rows of type 4 in the cohort the engine was given."""
        out = C.c_int64()
        _lib.check(self.lib.mmhn_get_unknown_rows(self.h, C.byref(out)))
        return int(out.value)

    # ---- argument checks of the single-vector primitives: everything the C side reads through a raw pointer has the
    # length it will read (make_joint / make_single read the whole state, build_params N x N / N entries, up() and down()
    # 2^k elements)
    def _state(self, state, joint=True):
        """int8 state of length 2n+1 (joint) or n+1 (single tumour) holding only 0 / 1, its pointer and k."""
        st = np.asarray(state)
        L = 2 * self.n + 1 if joint else self.N
        if st.ndim != 1 or st.shape[0] != L:
            raise ValueError(f"state must have shape ({L},), got {st.shape}")
        if not np.isin(st, (0, 1)).all():
            raise ValueError("state must hold only 0 and 1")
        st, sp = _s(st)
        return st, sp, int(st.sum())

    def _theta(self, log_theta):
        lt, ltp = _f(log_theta)
        if lt.shape != (self.N, self.N):
            raise ValueError(f"log_theta must have shape ({self.N}, {self.N}), got {lt.shape}")
        return lt, ltp

    def _rates(self, log_d, name="log_d"):
        d, dp_ = _f(log_d)
        if d.shape != (self.N,):
            raise ValueError(f"{name} must have shape ({self.N},), got {d.shape}")
        return d, dp_

    def _event(self, i):
        if isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)) or not 0 <= int(i) <= self.n:
            raise ValueError(f"i must be an event index in 0..{self.n}, got {i!r}")
        return int(i)

    # ---- joint primitives
    def kronvec(self, log_theta, p, state, diag=True, transpose=False):
        lt, ltp = self._theta(log_theta); st, sp, k = self._state(state); pv, pp = _vec(p, 2 ** k, "p")
        y = np.zeros_like(pv)
        _lib.check(self.lib.mmhn_kronvec(self.h, ltp, sp, pp, y.ctypes.data_as(f64p), int(diag), int(transpose)))
        return y

    def kronvec_batched(self, log_theta, p, state, diag=True, transpose=False):
        """kronvec for a batch p[b][2^k] of vectors of one restricted space: one launch, y[b][2^k]."""
        lt, ltp = self._theta(log_theta); st, sp, k = self._state(state)
        pv = np.ascontiguousarray(p, dtype=np.float64)
        if pv.ndim != 2 or pv.shape[1] != 2 ** k:
            raise ValueError("p must have shape [batch, 2^k]")
        y = np.zeros_like(pv)
        _lib.check(self.lib.mmhn_kronvec_batched(self.h, ltp, sp, int(pv.shape[0]), pv.ctypes.data_as(f64p),
                                                 y.ctypes.data_as(f64p), int(diag), int(transpose)))
        return y

    def jacobi_step_batched(self, log_theta, log_d_p, log_d_m, p, rhs, state, transpose=False):
        """One sweep of R_i_inv_vec's iteration for a batch: lidg * (Q_off p + rhs), shapes [batch, 2^k]."""
        keep, (ltp, ap, bp) = self._params(log_theta, log_d_p, log_d_m); st, sp, k = self._state(state)
        pv = np.ascontiguousarray(p, dtype=np.float64)
        rv = np.ascontiguousarray(rhs, dtype=np.float64)
        if pv.ndim != 2 or pv.shape != rv.shape or pv.shape[1] != 2 ** k:
            raise ValueError("p and rhs must have shape [batch, 2^k]")
        y = np.zeros_like(pv)
        _lib.check(self.lib.mmhn_jacobi_step_batched(self.h, ltp, ap, bp, sp, int(pv.shape[0]), pv.ctypes.data_as(f64p),
                                                     rv.ctypes.data_as(f64p), y.ctypes.data_as(f64p), int(transpose)))
        return y

    def kron_diag(self, log_theta, state):
        lt, ltp = self._theta(log_theta); st, sp, k = self._state(state)
        y = np.zeros(2 ** k)
        _lib.check(self.lib.mmhn_kron_diag(self.h, ltp, sp, y.ctypes.data_as(f64p)))
        return y

    def diag_scal(self, log_d, state, p, which):
        d, dp_ = self._rates(log_d); st, sp, k = self._state(state); pv, pp = _vec(p, 2 ** k, "p")
        y = np.zeros_like(pv)
        _lib.check(self.lib.mmhn_diag_scal(self.h, dp_, sp, pp, y.ctypes.data_as(f64p), int(which)))
        return y

    def obs_indices(self, state, pt_first):
        st, sp, k = self._state(state)
        n = self.n
        free = int(st[1:2 * n:2].sum()) if pt_first else int(st[0:2 * n:2].sum())
        idx = np.zeros(2 ** free, dtype=np.int64)
        cnt = C.c_int64()
        _lib.check(self.lib.mmhn_obs_states(self.h, sp, int(bool(pt_first)), idx.ctypes.data_as(i64p), C.byref(cnt)))
        return idx[:cnt.value]

    def resolvent(self, log_theta, log_d_p, log_d_m, x, state, transpose=False):
        keep, (a, b, c) = self._params(log_theta, log_d_p, log_d_m)
        st, sp, k = self._state(state); xv, xp = _vec(x, 2 ** k, "x")
        y = np.zeros_like(xv)
        _lib.check(self.lib.mmhn_resolvent(self.h, a, b, c, sp, xp, y.ctypes.data_as(f64p), int(transpose)))
        return y

    def x_partial_Q_y(self, log_theta, x, y, state):
        lt, ltp = self._theta(log_theta); st, sp, k = self._state(state)
        xv, xp = _vec(x, 2 ** k, "x"); yv, yp = _vec(y, 2 ** k, "y")
        G = np.zeros((self.N, self.N))
        _lib.check(self.lib.mmhn_x_partial_Q_y(self.h, ltp, sp, xp, yp, G.ctypes.data_as(f64p)))
        return G

    def x_partial_D_y(self, log_d_p, log_d_m, state, x, y):
        a, ap = self._rates(log_d_p, "log_d_p"); b, bp = self._rates(log_d_m, "log_d_m"); st, sp, k = self._state(state)
        xv, xp = _vec(x, 2 ** k, "x"); yv, yp = _vec(y, 2 ** k, "y")
        ddp, ddm = np.zeros(self.N), np.zeros(self.N)
        _lib.check(self.lib.mmhn_x_partial_D_y(self.h, ap, bp, sp, xp, yp, ddp.ctypes.data_as(f64p),
                                               ddm.ctypes.data_as(f64p)))
        return ddp, ddm

    def partial_diag_scal(self, log_d, state, p, i, which):
        d, dp_ = self._rates(log_d); st, sp, k = self._state(state); pv, pp = _vec(p, 2 ** k, "p")
        i = self._event(i)
        y = np.zeros_like(pv)
        _lib.check(self.lib.mmhn_partial_diag_scal(self.h, dp_, sp, pp, i, int(which), y.ctypes.data_as(f64p)))
        return y

    # ---- single-tumour primitives
    def v_kronvec(self, log_theta, p, state, diag=True, transpose=False):
        lt, ltp = self._theta(log_theta); st, sp, k = self._state(state, False); pv, pp = _vec(p, 2 ** k, "p")
        y = np.zeros_like(pv)
        _lib.check(self.lib.mmhn_v_kronvec(self.h, ltp, sp, pp, y.ctypes.data_as(f64p), int(diag), int(transpose)))
        return y

    def v_resolvent(self, log_theta, x, state, d_rates=None, transpose=False):
        lt, ltp = self._theta(log_theta); st, sp, k = self._state(state, False); xv, xp = _vec(x, 2 ** k, "x")
        y = np.zeros_like(xv)
        if d_rates is None or np.ndim(d_rates) == 0:
            if d_rates is not None and float(d_rates) != 1.0:
                d_rates = np.full_like(xv, float(d_rates))
            else:
                d_rates = None
        dr = None
        if d_rates is not None:
            dkeep, dr = _vec(d_rates, 2 ** k, "d_rates")
        _lib.check(self.lib.mmhn_v_resolvent(self.h, ltp, sp, dr, xp, y.ctypes.data_as(f64p), int(transpose)))
        return y

    def v_x_partial_Q_y(self, log_theta, x, y, state):
        lt, ltp = self._theta(log_theta); st, sp, k = self._state(state, False)
        xv, xp = _vec(x, 2 ** k, "x"); yv, yp = _vec(y, 2 ** k, "y")
        G, dd = np.zeros((self.N, self.N)), np.zeros(self.N)
        _lib.check(self.lib.mmhn_v_x_partial_Q_y(self.h, ltp, sp, xp, yp, G.ctypes.data_as(f64p),
                                                 dd.ctypes.data_as(f64p)))
        return G, dd

    def v_kron_diag(self, log_theta, state, diag=None):
        lt, ltp = self._theta(log_theta); st, sp, k = self._state(state, False)
        out = np.zeros(2 ** k)
        dg = None
        if diag is not None:
            dkeep, dg = _vec(diag, 2 ** k, "diag")
        _lib.check(self.lib.mmhn_v_kron_diag(self.h, ltp, sp, dg, out.ctypes.data_as(f64p)))
        return out

    def v_scal_d_pt(self, log_d_p, log_d_m, state, vec):
        a, ap = self._rates(log_d_p, "log_d_p"); b, bp = self._rates(log_d_m, "log_d_m")
        st, sp, k = self._state(state, False); v, vp = _vec(vec, 2 ** k, "vec")
        op, om = np.zeros_like(v), np.zeros_like(v)
        _lib.check(self.lib.mmhn_v_scal_d_pt(self.h, ap, bp, sp, vp, op.ctypes.data_as(f64p), om.ctypes.data_as(f64p)))
        return op, om

    def v_d_scal_d_pt(self, log_d_p, log_d_m, state, vec, i):
        a, ap = self._rates(log_d_p, "log_d_p"); b, bp = self._rates(log_d_m, "log_d_m")
        st, sp, k = self._state(state, False); v, vp = _vec(vec, 2 ** k, "vec")
        i = self._event(i)
        op, om = np.zeros_like(v), np.zeros_like(v)
        _lib.check(self.lib.mmhn_v_d_scal_d_pt(self.h, ap, bp, sp, vp, i, op.ctypes.data_as(f64p),
                                               om.ctypes.data_as(f64p)))
        return op, om

    def v_x_partial_D_y(self, log_d_p, log_d_m, state, x, y):
        a, ap = self._rates(log_d_p, "log_d_p"); b, bp = self._rates(log_d_m, "log_d_m")
        st, sp, k = self._state(state, False)
        xv, xp = _vec(x, 2 ** k, "x"); yv, yp = _vec(y, 2 ** k, "y")
        ddp, ddm = np.zeros(self.N), np.zeros(self.N)
        _lib.check(self.lib.mmhn_v_x_partial_D_y(self.h, ap, bp, sp, xp, yp, ddp.ctypes.data_as(f64p),
                                                 ddm.ctypes.data_as(f64p)))
        return ddp, ddm

    # ---- patient shards on several GPUs
    def comm_init(self, unique_id: bytes, rank: int, n_ranks: int):
        """Join the RCCL communicator `unique_id` (from `unique_id()` on rank 0); afterwards cohort_sums / score /
        score_and_grad return the sums over all ranks (one all-reduce on the engine's stream per call)."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _lib.check(self.lib.mmhn_comm_init(self.h, buf, int(rank), int(n_ranks)))
        self.comm_size = int(n_ranks)

    def comm_destroy(self):
        _lib.check(self.lib.mmhn_comm_destroy(self.h))
        self.comm_size = 1

    # ---- simulation
    def simulate(self, log_theta, pt_d_ef, mt_d_ef, n_sim, seed=0, orders=False):
        """Gillespie samples: int8 dat [n_sim, 2n+2] (and the event sequences [n_sim, 2N+2] if `orders`)."""
        lt, ltp = _f(log_theta); a, ap = _f(pt_d_ef); b, bp = _f(mt_d_ef)
        n_sim = int(n_sim)
        dat = np.zeros((n_sim, 2 * self.n + 2), dtype=np.int8)
        od = np.zeros((n_sim, 2 * self.N + 2), dtype=np.int8) if orders else None
        _lib.check(self.lib.mmhn_simulate(self.h, ltp, ap, bp, n_sim, int(seed) & (2 ** 64 - 1),
                                          dat.ctypes.data_as(_lib.i8p),
                                          od.ctypes.data_as(_lib.i8p) if orders else None))
        return (dat, od) if orders else dat

    def simulate_summary(self, log_theta, pt_d_ef, mt_d_ef, n_sim, seed=0, first=0):
        """Counts of the Gillespie samples [first, first + n_sim) without the samples (mmhn_simulate_summary): int64
        [4 + 5n] = n_sim, seeded, PT first, MT first, then per mutation pre, pt, mt, shared (seeded) and pt_nm
        (unseeded); include/metmhn_amd.h has the layout."""
        lt, ltp = self._theta(log_theta); a, ap = self._rates(pt_d_ef, "pt_d_ef"); b, bp = self._rates(mt_d_ef, "mt_d_ef")
        n_sim, first = int(n_sim), int(first)
        if n_sim < 0 or first < 0:
            raise ValueError(f"n_sim and first must be non-negative, got n_sim={n_sim}, first={first}")
        counts = np.zeros(4 + 5 * self.n, dtype=np.int64)
        _lib.check(self.lib.mmhn_simulate_summary(self.h, ltp, ap, bp, first, n_sim, int(seed) & (2 ** 64 - 1),
                                                  counts.ctypes.data_as(i64p)))
        return counts

    def simulate_pairs(self, log_theta, pt_d_ef, mt_d_ef, n_sim, seed=0, first=0):
        """Pairwise co-occurrence and burden counts of the Gillespie samples [first, first + n_sim) without the samples
        (mmhn_simulate_pairs): int64 n_class [3], pairs [3, 2n, 2n] (per class G.T @ G of simulate's genotype columns) and
        burden [3, 5, n+1] (histograms of |PT|, |MT|, |PT & MT|, |PT & ~MT|, |MT & ~PT|); classes 0 unseeded, 1 seeded
        and PT observed first, 2 seeded and MT observed first; include/metmhn_amd.h has the definition."""
        lt, ltp = self._theta(log_theta); a, ap = self._rates(pt_d_ef, "pt_d_ef"); b, bp = self._rates(mt_d_ef, "mt_d_ef")
        n_sim, first = int(n_sim), int(first)
        if n_sim < 0 or first < 0:
            raise ValueError(f"n_sim and first must be non-negative, got n_sim={n_sim}, first={first}")
        n_class = np.zeros(3, dtype=np.int64)
        pairs = np.zeros((3, 2 * self.n, 2 * self.n), dtype=np.int64)
        burden = np.zeros((3, 5, self.n + 1), dtype=np.int64)
        _lib.check(self.lib.mmhn_simulate_pairs(self.h, ltp, ap, bp, first, n_sim, int(seed) & (2 ** 64 - 1),
                                                n_class.ctypes.data_as(i64p), pairs.ctypes.data_as(i64p),
                                                burden.ctypes.data_as(i64p)))
        return n_class, pairs, burden

    # ---- likeliest event orders
    def likeliest_orders(self, log_theta, obs1, obs2, dat, front_cap=0):
        """MetMHN.likeliest_order of every row of a reference-format `dat` [n_pat, 2n+3] in one call
        (mmhn_likeliest_orders): int8 orders [n_pat, 2N-1] padded with -1, float64 prob [n_pat], int32 status [n_pat]
        (0 ok, 1 front overflow, 2 invalid row - reason code in orders[i, 0] -, 3 lattice larger than the workspace)."""
        lt, ltp = _f(log_theta); a, ap = _f(obs1); b, bp = _f(obs2)
        d = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
        if d.ndim != 2:
            raise ValueError("dat must be a 2-D array [n_pat, 2 n_mut + 3]")
        n_pat = d.shape[0]
        orders = np.full((n_pat, 2 * self.N - 1), -1, dtype=np.int8)
        prob = np.zeros(n_pat)
        status = np.zeros(n_pat, dtype=np.int32)
        _lib.check(self.lib.mmhn_likeliest_orders(self.h, ltp, ap, bp, d.ctypes.data_as(i8p), n_pat, int(d.shape[1]),
                                                  int(front_cap), orders.ctypes.data_as(i8p), prob.ctypes.data_as(f64p),
                                                  status.ctypes.data_as(_lib.i32p)))
        return orders, prob, status

    def _order_rows(self, fn, log_theta, obs1, obs2, dat, *shapes, dtypes=None):
        """One call of an mmhn_order_* entry point `fn` on a reference-format `dat`: log_evidence [n_pat], one array
        [n_pat, *shape] per result of the entry point (float64, or the int8 / int32 / float64 of `dtypes`), int32 status
        [n_pat]."""
        keep, (ltp, ap, bp) = self._params(log_theta, obs1, obs2)
        d = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
        if d.ndim != 2:
            raise ValueError("dat must be a 2-D array [n_pat, 2 n_mut + 3]")
        n_pat = d.shape[0]
        kinds = dtypes or (np.float64,) * len(shapes)
        # (the library fills them with NaN / -1 first)
        out = [np.zeros(n_pat)] + [np.empty((n_pat,) + shape, dtype=kind) for shape, kind in zip(shapes, kinds)]
        status = np.zeros(n_pat, dtype=np.int32)
        ptr = {np.dtype(np.float64): f64p, np.dtype(np.int8): i8p, np.dtype(np.int32): _lib.i32p}
        _lib.check(fn(self.h, ltp, ap, bp, d.ctypes.data_as(i8p), n_pat, int(d.shape[1]),
                      *(a.ctypes.data_as(ptr[a.dtype]) for a in out), status.ctypes.data_as(_lib.i32p)))
        return (*out, status)

    def order_posteriors(self, log_theta, obs1, obs2, dat):
        """MetMHN.order_posterior of every row of a reference-format `dat` [n_pat, 2n+3] in one call
        (mmhn_order_posteriors): float64 log_evidence [n_pat], pre [n_pat, n], seed_pos [n_pat, N], int32 status [n_pat]
        (low half 0 ok, 2 invalid row - reason code in status >> 16 -, 3 lattice larger than the workspace; NaN outputs
        wherever it is not 0, and in pre / seed_pos of the "absent" rows)."""
        return self._order_rows(self.lib.mmhn_order_posteriors, log_theta, obs1, obs2, dat, (self.n,), (self.N,))

    def order_precedences(self, log_theta, obs1, obs2, dat):
        """MetMHN.order_precedence of every row of a reference-format `dat` [n_pat, 2n+3] in one call
        (mmhn_order_precedences): float64 log_evidence [n_pat], prec [n_pat, 2n+1, 2n+1] over the event codes (NaN where
        a code is not in the row), int32 status [n_pat] (low half 0 ok, 2 invalid row - reason code in status >> 16 -,
        3 lattice larger than the workspace; NaN outputs wherever it is not 0)."""
        L = 2 * self.n + 1
        return self._order_rows(self.lib.mmhn_order_precedences, log_theta, obs1, obs2, dat, (L, L))

    def order_positions(self, log_theta, obs1, obs2, dat):
        """MetMHN.order_position of every row of a reference-format `dat` [n_pat, 2n+3] in one call
        (mmhn_order_positions): float64 log_evidence [n_pat], pos_pt and pos_mt [n_pat, N, N] (event, position; NaN for an
        event the row does not carry in that lineage), int32 status [n_pat] (low half 0 ok, 2 invalid row - reason code in
        status >> 16 -, 3 lattice larger than the workspace; NaN outputs wherever it is not 0)."""
        NN = (self.N, self.N)
        return self._order_rows(self.lib.mmhn_order_positions, log_theta, obs1, obs2, dat, NN, NN)

    def order_times(self, log_theta, obs1, obs2, dat):
        """MetMHN.order_time of every row of a reference-format `dat` [n_pat, 2n+3] in one call (mmhn_order_times): float64
        log_evidence [n_pat], time [n_pat, 2n+1] over the event codes (NaN where a code is not in the row), obs [n_pat, 2]
        (first, second observation; a one-tumour row has one), pt_first [n_pat] (NaN for a one-tumour row), int32 status
        [n_pat] (low half 0 ok, 2 invalid row - reason code in status >> 16 -, 3 lattice larger than the workspace; NaN
        outputs wherever it is not 0)."""
        return self._order_rows(self.lib.mmhn_order_times, log_theta, obs1, obs2, dat, (2 * self.n + 1,), (2,), ())

    def order_snapshots(self, log_theta, obs1, obs2, dat):
        """MetMHN.order_snapshot of every row of a reference-format `dat` [n_pat, 2n+3] in one call (mmhn_order_snapshots):
        float64 log_evidence [n_pat], held [n_pat, 2, 2n+1] over the event codes (NaN where a code is not in the row), late
        [n_pat, 2, N], int8 map_state [n_pat, 2n+1], int32 map_first [n_pat], float64 map_prob [n_pat] (NaN / -1 throughout a
        one-tumour row, which has no first observation), int32 status [n_pat] (low half 0 ok, 2 invalid row - reason code in
        status >> 16 -, 3 lattice larger than the workspace; NaN / -1 outputs wherever it is not 0)."""
        L = 2 * self.n + 1
        return self._order_rows(self.lib.mmhn_order_snapshots, log_theta, obs1, obs2, dat, (2, L), (2, self.N), (L,), (), (),
                                dtypes=(np.float64, np.float64, np.int8, np.int32, np.float64))

    def order_samples(self, log_theta, obs1, obs2, dat, n_samples, seed=0, first=0):
        """MetMHN.sample_order of every row of a reference-format `dat` [n_pat, 2n+3] in one call (mmhn_order_samples), row
        i with row=i, the sample indices first ... first + n_samples - 1 under the 64-bit `seed`: float64 log_evidence
        [n_pat], int8 orders [n_pat, n_samples, 2n+1] padded with -1, float64 log_prob [n_pat, n_samples], int32 status
        [n_pat] (low half 0 ok, 2 invalid row - reason code in status >> 16 -, 3 lattice and samples larger than the
        workspace; orders -1 and log_prob NaN wherever it is not 0)."""
        keep, (ltp, ap, bp) = self._params(log_theta, obs1, obs2)
        d = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
        if d.ndim != 2:
            raise ValueError("dat must be a 2-D array [n_pat, 2 n_mut + 3]")
        n_samples, first = int(n_samples), int(first)
        if n_samples < 0 or first < 0:
            raise ValueError(f"n_samples and first must be non-negative, got n_samples={n_samples}, first={first}")
        n_pat = d.shape[0]
        le = np.zeros(n_pat)
        orders = np.empty((n_pat, n_samples, 2 * self.n + 1), dtype=np.int8)      # (the library fills them first)
        log_prob = np.empty((n_pat, n_samples))
        status = np.zeros(n_pat, dtype=np.int32)
        _lib.check(self.lib.mmhn_order_samples(self.h, ltp, ap, bp, d.ctypes.data_as(i8p), n_pat, int(d.shape[1]), first,
                                               n_samples, int(seed) & (2 ** 64 - 1), le.ctypes.data_as(f64p),
                                               orders.ctypes.data_as(i8p), log_prob.ctypes.data_as(f64p),
                                               status.ctypes.data_as(_lib.i32p)))
        return le, orders, log_prob, status

    # ---- seeding forecasts
    def seeding_forecasts(self, log_theta, obs1, genotypes, until="seeding"):
        """MetMHN.seeding_forecast of every row of int8 `genotypes` [R, n] (1 = held) in one call (mmhn_seeding_forecasts),
        until "seeding" or "observation": float64 p_seed [R], time [R], before [R, n], with_seed [R, n] (NaN for a held
        mutation), n_before [R, n+1] (0 past the row's free mutations), int32 status [R] (low half 0 ok, 2 an entry other than
        0 / 1 - reason code 8 in status >> 16 -, 3 more than 30 free mutations or a lattice larger than the workspace; NaN
        outputs wherever it is not 0)."""
        if until not in ("seeding", "observation"):
            raise ValueError("until must be 'seeding' or 'observation'")
        lt, ltp = self._theta(log_theta); a, ap = self._rates(obs1, "obs1")
        g = np.ascontiguousarray(np.asarray(genotypes).astype(np.int8))
        if g.ndim != 2 or g.shape[1] != self.n:
            raise ValueError(f"genotypes must be a 2-D array [R, {self.n}]")
        R = g.shape[0]
        p_seed, time = np.empty(R), np.empty(R)                 # (the library fills them with NaN first)
        before, with_seed, n_before = np.empty((R, self.n)), np.empty((R, self.n)), np.empty((R, self.N))
        status = np.zeros(R, dtype=np.int32)
        _lib.check(self.lib.mmhn_seeding_forecasts(
            self.h, ltp, ap, g.ctypes.data_as(i8p), R, 0 if until == "seeding" else 1, p_seed.ctypes.data_as(f64p),
            time.ctypes.data_as(f64p), before.ctypes.data_as(f64p), with_seed.ctypes.data_as(f64p),
            n_before.ctypes.data_as(f64p), status.ctypes.data_as(_lib.i32p)))
        return p_seed, time, before, with_seed, n_before, status

    # ---- sweeps over all 2^n genotypes
    def _lattice_call(self, genotypes, planes, summary, full, call):
        """What the three whole-lattice calls share: the check of int8 `genotypes` [R, n], the buffers values [R, planes],
        status [R], sums (with `summary`) and whole [planes, 2^n] (with `full`), the library call - call(genotypes, R,
        values, status, sums or None, whole or None), all pointers - and the summary split into (mass [2], pairs [2, n, n],
        burden [2, n+1]).  Returns values, status, sums, whole."""
        g = np.ascontiguousarray(np.asarray(genotypes).astype(np.int8))
        if g.ndim != 2 or g.shape[1] != self.n:
            raise ValueError(f"genotypes must be a 2-D array [R, {self.n}]")
        R, n = g.shape[0], self.n
        values = np.empty((R, planes))                           # (the library fills it with NaN first)
        status = np.zeros(R, dtype=np.int32)
        sums = np.empty((2, 1 + n * n + n + 1)) if summary else None
        whole = np.empty((planes, 1 << n)) if full else None
        _lib.check(call(g.ctypes.data_as(i8p), R, values.ctypes.data_as(f64p), status.ctypes.data_as(_lib.i32p),
                        sums.ctypes.data_as(f64p) if summary else None, whole.ctypes.data_as(f64p) if full else None))
        if summary:
            sums = (np.ascontiguousarray(sums[:, 0]), np.ascontiguousarray(sums[:, 1:1 + n * n]).reshape(2, n, n),
                    np.ascontiguousarray(sums[:, 1 + n * n:]))
        return values, status, sums, whole

    # ---- seeding landscape
    def seeding_landscape(self, log_theta, obs1, genotypes, until="seeding", full=False):
        """The four forecast scalars of every genotype of the model from one backward sweep over all 2^n genotype codes
        (mmhn_seeding_landscape), until "seeding" or "observation", read at the rows of int8 `genotypes` [R, n] (1 = held; R
        may be 0): float64 values [R, 4] = p_seed, time, new_events, seed_events, int32 status [R] (0 ok, 2 with reason code
        8 in status >> 16 for an entry other than 0 / 1, whose values are NaN), and with full=True the whole landscape
        [4, 2^n] by code (bit j = mutation j), else None.  Raises when 32 B x 2^n and the tile list exceed the workspace
        limit."""
        if until not in ("seeding", "observation"):
            raise ValueError("until must be 'seeding' or 'observation'")
        lt, ltp = self._theta(log_theta); a, ap = self._rates(obs1, "obs1")
        values, status, _, whole = self._lattice_call(
            genotypes, 4, False, full, lambda gp, R, vp, sp, _, wp: self.lib.mmhn_seeding_landscape(
                self.h, ltp, ap, 0 if until == "seeding" else 1, gp, R, vp, sp, wp))
        return values, status, whole

    # ---- genotype distribution
    def genotype_distribution(self, log_theta, obs1, genotypes, summary=True, full=False):
        """The probability of every genotype to be the primary tumour's observed one, unseeded (U) and seeded by then (S),
        from one forward sweep over all 2^n genotype codes (mmhn_genotype_distribution), read at the rows of int8
        `genotypes` [R, n] (1 = held; R may be 0): float64 values [R, 2] = U, S, int32 status [R] (0 ok, 2 with reason code
        8 in status >> 16 for an entry other than 0 / 1, whose values are NaN), with summary=True (mass [2], pairs [2, n, n],
        burden [2, n+1]) of the planes U and S, else None, and with full=True the two planes [2, 2^n] by code (bit j =
        mutation j), else None.  Raises when 16 B x 2^n, the tile list and the tiles' partial sums exceed the workspace
        limit."""
        lt, ltp = self._theta(log_theta); a, ap = self._rates(obs1, "obs1")
        return self._lattice_call(genotypes, 2, summary, full,
                                  lambda *buffers: self.lib.mmhn_genotype_distribution(self.h, ltp, ap, *buffers))

    # ---- metastasis distribution
    def metastasis_distribution(self, log_theta, obs1, obs2, genotypes, summary=True, full=False):
        """The probability of every genotype to be the founder's (Z: the seeding happens before the PT's observation and the
        seeding cell holds exactly that genotype), the metastasis' observed one (M, exp(lp) of the type-2 row) and M weighted
        by the number of its mutations the founder held (C), from one forward sweep over all 2^n genotype codes
        (mmhn_metastasis_distribution), read at the rows of int8 `genotypes` [R, n] (1 = held; R may be 0): float64 values
        [R, 3] = Z, M, C, int32 status [R] (0 ok, 2 with reason code 8 in status >> 16 for an entry other than 0 / 1, whose
        values are NaN), with summary=True (mass [2], pairs [2, n, n], burden [2, n+1]) of the planes Z and M, else None, and
        with full=True the three planes [3, 2^n] by code (bit j = mutation j), else None.  Raises when 24 B x 2^n, the tables,
        the tile list and the tiles' partial sums exceed the workspace limit."""
        lt, ltp = self._theta(log_theta); a, ap = self._rates(obs1, "obs1"); b, bp = self._rates(obs2, "obs2")
        return self._lattice_call(genotypes, 3, summary, full,
                                  lambda *buffers: self.lib.mmhn_metastasis_distribution(self.h, ltp, ap, bp, *buffers))

    # ---- partner distributions
    def partner_distributions(self, log_theta, obs1, obs2, genotypes, given="PT", targets=None, summary=True, full=False):
        """For every row of int8 `genotypes` [R, n] (1 = held; R may be 0), taken as the primary tumour observed seeded
        (given="PT") or as the metastasis (given="MT"), the joint probability with every genotype of the other tumour and
        with every founder (mmhn_partner_distributions; a backward pass over the subsets of the row and one forward sweep
        over all 2^n codes per DISTINCT row): float64 values [R, 3] = mass (the sum of the joint), founder W and joint J at
        the row of `targets` [R, n] (NaN without targets), int32 status [R] (0 ok, 2 with reason code 8 in status >> 16 for
        an entry of the row or its target other than 0 / 1, whose outputs are NaN), with summary=True (mass [R, 2], pairs
        [R, 2, n, n], burden [R, 2, n+1]) of the founder and the partner plane of every row, else None, and with full=True,
        which needs R == 1, the two planes [2, 2^n] by code, else None.  Raises when 16 B x 2^n, the tables, the tile
        lists and the tiles' partial sums exceed the workspace limit."""
        if given not in ("PT", "MT"):
            raise ValueError("given must be 'PT' or 'MT'")
        lt, ltp = self._theta(log_theta); a, ap = self._rates(obs1, "obs1"); b, bp = self._rates(obs2, "obs2")
        n = self.n
        g = np.ascontiguousarray(np.asarray(genotypes).astype(np.int8))
        if g.ndim != 2 or g.shape[1] != n:
            raise ValueError(f"genotypes must be a 2-D array [R, {n}]")
        R = g.shape[0]
        t = None
        if targets is not None:
            t = np.ascontiguousarray(np.asarray(targets).astype(np.int8))
            if t.shape != g.shape:
                raise ValueError(f"targets must be a 2-D array [R, {n}] with a row per genotype")
        if full and R != 1:
            raise ValueError(f"full=True returns the planes of one query: genotypes must have one row, got {R}")
        values = np.empty((R, 3))                                # (the library fills it with NaN first)
        status = np.zeros(R, dtype=np.int32)
        sums = np.empty((R, 2, 1 + n * n + n + 1)) if summary else None
        whole = np.empty((2, 1 << n)) if full else None
        _lib.check(self.lib.mmhn_partner_distributions(
            self.h, ltp, ap, bp, 0 if given == "PT" else 1, g.ctypes.data_as(i8p),
            t.ctypes.data_as(i8p) if t is not None else None, R, values.ctypes.data_as(f64p),
            status.ctypes.data_as(_lib.i32p), sums.ctypes.data_as(f64p) if summary else None,
            whole.ctypes.data_as(f64p) if full else None))
        if summary:
            sums = (np.ascontiguousarray(sums[:, :, 0]), np.ascontiguousarray(sums[:, :, 1:1 + n * n]).reshape(R, 2, n, n),
                    np.ascontiguousarray(sums[:, :, 1 + n * n:]))
        return values, status, sums, whole

    # ---- cross table
    def cross_table(self, log_theta, obs1, obs2, burden=True):
        """The exact second moments of the (PT x MT) table (mmhn_cross_table; one forward plane for the founder, a backward
        sweep of four planes per block of four features of either chain, a fold per pair of blocks), all joint with
        "seeded": float64 mass, pt [n], mt [n], cross [n, n] = P(PT holds i, MT holds j, seeded), burden [n+1, n+1] =
        P(|PT| = k, |MT| = l, seeded), gene_burden [2, n, n+1] (PT gene i against |MT| = l, MT gene j against |PT| = k).
        burden=False sweeps the n gene features only: burden and gene_burden are NaN, the rest has the same bytes.  An fp64
        engine only.  Raises when 72 B x 2^n, the tables, the tile list and the tiles' partial sums exceed the workspace
        limit; above that the planes that fit are held and the others swept again, with the same bytes."""
        if getattr(self, "dtype", "f64") != "f64":
            raise ValueError("the cross table needs an fp64 engine (dtype='f64')")
        lt, ltp = self._theta(log_theta); a, ap = self._rates(obs1, "obs1"); b, bp = self._rates(obs2, "obs2")
        n = self.n
        out = np.empty(1 + 2 * n + n * n + (n + 1) * (n + 1) + 2 * n * (n + 1))      # (the library fills it with NaN first)
        _lib.check(self.lib.mmhn_cross_table(self.h, ltp, ap, bp, 1 if burden else 0, out.ctypes.data_as(f64p)))
        at = np.cumsum([0, 1, n, n, n * n, (n + 1) * (n + 1), 2 * n * (n + 1)])
        mass, pt, mt, cross, bur, gb = (out[at[k]:at[k + 1]].copy() for k in range(6))
        return float(mass[0]), pt, mt, cross.reshape(n, n), bur.reshape(n + 1, n + 1), gb.reshape(2, n, n + 1)

    # ---- measurement
    def bench_kronvec(self, log_theta, state, batch, iters, transpose=False, jacobi=False, tiles=False):
        """ms per launch of mmhn_kronvec_batched's launch (or the fused Jacobi step); tiles=True also returns
        (tiles with entries of Q_off, tiles per launch)."""
        lt, ltp = _f(log_theta); st, sp = _s(state)
        ms = C.c_double()
        tl = (C.c_int64 * 2)()
        _lib.check(self.lib.mmhn_bench_kronvec(self.h, ltp, sp, int(batch), int(iters), int(transpose), int(jacobi),
                                               C.byref(ms), tl))
        return (ms.value, int(tl[0]), int(tl[1])) if tiles else ms.value

    def bench_stream(self, nbytes=1 << 30, iters=10, kind="copy"):
        """Measured device-memory bandwidth (GB/s) of a plain copy / triad stream on this GPU."""
        out = C.c_double()
        _lib.check(self.lib.mmhn_bench_stream(self.h, int(nbytes), int(iters), 0 if kind == "copy" else 1, C.byref(out)))
        return out.value

    def counters(self):
        c = _lib.Counters()
        _lib.check(self.lib.mmhn_get_counters(self.h, C.byref(c)))
        out = {"eval_ms": c.eval_ms, "evals": c.evals, "comm_ranks": int(c.comm_ranks), "comm_rank": int(c.comm_rank)}
        for i, name in enumerate(_lib.KERNEL_CLASSES):
            k = c.kernel[i]
            out[name] = {"ms": k.ms, "launches": k.launches, "alg_bytes": k.alg_bytes}
        return out

    def reset_counters(self):
        _lib.check(self.lib.mmhn_reset_counters(self.h))

    def debug_lane_moves(self, transposed=False):
        """out[i][lane] = source lane of the window solve's exchange along lane bit i (csrc/wsolve.h)."""
        out = (C.c_int * (6 * 64))()
        _lib.check(self.lib.mmhn_debug_lane_moves(self.h, int(bool(transposed)), out))
        return np.array(out[:], dtype=np.int64).reshape(6, 64)
