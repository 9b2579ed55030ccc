"""Every single-vector primitive against a high-precision reference, across the tile boundary.

The 15 entry points of the reference's module surface (jx.kronvec, jx.likelihood, jx.vanilla -> Engine.kronvec ...
Engine.v_x_partial_D_y -> the api_* paths of csrc/prims.h) are swept over k = 0 .. 18, past the 12 tile bits
(MMHN_TB), on unseeded joint states and on joint states with one tumour plus seeding, at the largest event count
(n = 31: the last slots of a joint state and the last events of a single-tumour one), on fp64 and fp32 engines, under
both solvers, and with MMHN_POISON=1 on half of the cases: a poisoned engine NaN-fills every result buffer as soon as it
is allocated, so an element that no launch or memset writes shows in the output.

References: oracle/metmhn_oracle.py (pinned to the reference's golden vectors) on the GPU; oracle/dense.py's
first-principles dense generator in long double pins the oracle itself (CPU part, unmarked) at the states the golden
files lack - k = 0, unseeded, PT-only / MT-only with seeding.

Error bounds are componentwise, u = 2^-53 (fp64) or 2^-24 (fp32, against the fp64 reference):
- Q p: Q's off-diagonal rates are non-negative, so m = Q_off |p| + |diag Q| |p| bounds every term of y[x].  A rate is
  a product of at most k + 2 factors and y[x] a sum of at most k + 2N + 1 terms (N events):
  |y - y_ref| <= C_KV (k + N) u m.  Diagonal products (kron_diag, diag_scal, partial_diag_scal, scal_d_pt) take
  m = |y_ref|.
- Resolvent: D_obs - Q is a triangular M-matrix, so for x >= 0 every term of the solution is non-negative and the
  error of each element is relative, accumulated over at most k + 1 levels: |y - y_ref| <= C_R (k + 1)(k + N) u R|x|.
  A signed x is bounded against the resolvent of |x|.
- Gradient entries (x_partial_*; x, y >= 0 as in the likelihood): rtol 1e-12 (fp64) / 1e-5 (fp32) with an atol of
  rtol times the largest entry of the same row of the reference G.
Indices (obs_states) are compared bit-exact.
"""
import os
import zlib

import numpy as np
import pytest

from oracle import dense as D
from oracle import metmhn_oracle as O

TB = 12                  # MMHN_TB, csrc/common.h
C_KV = 16                # products with Q and diagonal products, see the module docstring
C_R = 16                 # resolvents
RTOL_G = {"f64": 1e-12, "f32": 1e-5}
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ states and cases
def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


N_TOP = 31               # the largest event count (MAXN = 32 events with the seeding, csrc/desc.h)


def joint_state(layout, k, rng):
    """(n, int8 state [2n+1]) with exactly k active slots; two events stay inactive.

    seeded: seeding + a mix of pairs and lone PT / MT slots; unseeded: the same without seeding; pt_seed / mt_seed: one
    tumour + seeding; paired: pairs only (+ seeding when k is odd); lone: lone PT / MT slots + seeding; top: n = 31, the
    pairs of the events 0 - 2 and 28 - 30 and the seeding (slots 0 - 5 and 56 - 62, k = 13: one bit past the tile)."""
    if layout == "top":
        st = np.zeros(2 * N_TOP + 1, dtype=np.int8)
        st[[0, 1, 2, 3, 4, 5, 56, 57, 58, 59, 60, 61, 62]] = 1
        assert k == 13
        return N_TOP, st
    seed = layout in ("seeded", "pt_seed", "mt_seed", "lone") or (layout == "paired" and k % 2 == 1)
    if k == 0:
        seed = False
    r = k - int(seed)
    if layout in ("seeded", "unseeded"):
        pairs = r // 3
    elif layout == "paired":
        pairs = r // 2
    else:
        pairs = 0
    lone = r - 2 * pairs
    n = pairs + lone + 2
    st = np.zeros(2 * n + 1, dtype=np.int8)
    ev = rng.permutation(n)
    for j in ev[:pairs]:
        st[2 * j] = st[2 * j + 1] = 1
    for c, j in enumerate(ev[pairs:pairs + lone]):
        tum = {"pt_seed": 0, "mt_seed": 1}.get(layout, c % 2)
        st[2 * j + tum] = 1
    st[2 * n] = int(seed)
    assert int(st.sum()) == k
    return n, st


def single_state(layout, k, rng):
    """(n, int8 state [n+1]) with k active events; two events stay inactive.  seeded: the seeding event is one of them;
    top: n = 31, the events 0 - 9, 29, 30 and the seeding (event 31), k = 13."""
    if layout == "top":
        st = np.zeros(N_TOP + 1, dtype=np.int8)
        st[list(range(10)) + [29, 30, 31]] = 1
        assert k == 13
        return N_TOP, st
    seed = layout == "seeded" and k > 0
    n = max(k, 1) + 1
    st = np.zeros(n + 1, dtype=np.int8)
    st[rng.permutation(n)[:k - int(seed)]] = 1
    st[n] = int(seed)
    assert int(st.sum()) == k
    return n, st


JOINT_LAYOUTS_LARGE = ("seeded", "unseeded", "pt_seed", "mt_seed", "paired", "lone")


def _joint_cases():
    out = []
    for k in (0, 1, 2, 5, 11, 12, 13, 14, 16, 18):
        if k == 0:
            lays = ("unseeded",)
        elif k <= 2:
            lays = ("seeded", "unseeded", "pt_seed", "mt_seed")
        elif k <= TB or k == 18:
            lays = ("seeded", "unseeded")
        else:
            lays = JOINT_LAYOUTS_LARGE
        seen = set()
        for lay in lays:
            n, st = joint_state(lay, k, _rng(f"joint-{k}-{lay}"))
            key = (n, st.tobytes())
            if key in seen:
                continue
            seen.add(key)
            out.append((f"joint-k{k}-{lay}", k, lay))
    out.append(("joint-k13-top", 13, "top"))                     # (last: the poisoned half of the cases above stays as it was)
    return out


def _single_cases():
    out = []
    for k in (0, 1, 5, 11, 12, 13, 14, 16):
        for lay in (("unseeded",) if k == 0 else ("seeded", "unseeded")):
            out.append((f"single-k{k}-{lay}", k, lay))
    out.append(("single-k13-top", 13, "top"))
    return out


FP32_K = (5, 12, 13, 16)


def _with_modes(cases):
    """(id, k, layout, dtype, poison): every case in fp64, the k in FP32_K also in fp32; every other case of the list is
    run on poisoned engines, and every joint `lone` case with k > TB (seeding above the tile bits next to slots whose
    seed = 0 tiles have no entries of Q_off: the dead tiles api_kronvec does not launch)."""
    out = []
    for idx, (cid, k, lay) in enumerate(cases):
        poison = idx % 2 == 1 or (cid.startswith("joint") and lay == "lone" and k > TB)
        for dt in (("f64", "f32") if k in FP32_K else ("f64",)):
            tag = cid + ("-f32" if dt == "f32" else "") + ("-poison" if poison else "")
            out.append(pytest.param(cid, k, lay, dt, poison, id=tag))
    return out


# ------------------------------------------------------------------------------------------------ comparisons
class Checker:
    """Collects every violation of a case, so that one run reports all of them."""

    def __init__(self, tag):
        self.tag = tag
        self.fails = []
        self.worst = 0.0

    def _report(self, name, y, ref, err, bnd):
        bad = ~(err <= bnd)
        if bad.any():
            i = int(np.argmax(np.where(bad, np.nan_to_num(err - bnd, nan=np.inf), -np.inf)))
            self.fails.append(f"{self.tag} {name}: {int(bad.sum())}/{bad.size} elements out of bound; worst at {i}: "
                              f"got {y.flat[i]!r}, reference {ref.flat[i]!r}, bound {bnd.flat[i]:.3e}")
        pos = bnd > 0
        if pos.any() and np.isfinite(err).all():
            self.worst = max(self.worst, float(np.max(err[pos] / bnd[pos])))

    def bound(self, name, y, ref, bnd):
        """|y - ref| <= bnd elementwise (NaN anywhere fails)."""
        y, ref, bnd = (np.asarray(a, dtype=np.float64) for a in (y, ref, bnd))
        if y.shape != ref.shape:
            self.fails.append(f"{self.tag} {name}: shape {y.shape} != {ref.shape}")
            return
        if not np.isfinite(y).all():
            self.fails.append(f"{self.tag} {name}: {int((~np.isfinite(y)).sum())} non-finite elements (unwritten output)")
            return
        self._report(name, y, ref, np.abs(y - ref), bnd)

    def rows(self, name, G, ref, rtol):
        """Gradient entries: rtol per element plus rtol times the largest entry of the same row of ref."""
        G, ref = np.atleast_2d(np.asarray(G, dtype=np.float64)), np.atleast_2d(np.asarray(ref, dtype=np.float64))
        atol = rtol * np.abs(ref).max(axis=1, keepdims=True)
        self.bound(name, G, ref, rtol * np.abs(ref) + atol)

    def exact(self, name, got, ref):
        if not np.array_equal(np.asarray(got), np.asarray(ref)):
            self.fails.append(f"{self.tag} {name}: not bit-exact ({np.asarray(got)[:8]} vs {np.asarray(ref)[:8]} ...)")

    def raises(self, name, fn, exc=RuntimeError):
        try:
            fn()
        except exc:
            return
        except Exception as e:                                  # noqa: BLE001
            self.fails.append(f"{self.tag} {name}: raised {type(e).__name__} instead of {exc.__name__}: {e}")
            return
        self.fails.append(f"{self.tag} {name}: did not raise")

    def done(self):
        print(f"{self.tag}: worst error / bound = {self.worst:.3g}")
        assert not self.fails, "\n".join(self.fails)


# ------------------------------------------------------------------------------------------------ references
_REFS = {}


def _joint_inputs(cid, k, lay):
    rng = _rng(cid)
    n, st = joint_state(lay, k, _rng(f"joint-{k}-{lay}"))
    from metmhn_amd import synthetic
    lt, dp, dm = synthetic.random_params(n, seed=zlib.crc32(cid.encode()) % 100000)
    V = 2 ** k
    p, x = rng.normal(size=V), rng.normal(size=V)
    xg, yg = rng.random(V) + 0.1, rng.random(V) + 0.1
    return n, st, lt, dp, dm, p, x, xg, yg


def joint_refs(cid, k, lay):
    if cid in _REFS:
        return _REFS[cid]
    n, st, lt, dp, dm, p, x, xg, yg = _joint_inputs(cid, k, lay)
    r = {"in": (n, st, lt, dp, dm, p, x, xg, yg)}
    ap = np.abs(p)
    r["kd"] = O.kron_diag(lt, st, k)
    for tr in (False, True):
        off = O.kronvec(lt, ap, st, False, tr)
        r["m", False, tr] = off
        r["m", True, tr] = off + np.abs(r["kd"]) * ap
        for dg in (False, True):
            r["kv", dg, tr] = O.kronvec(lt, p, st, dg, tr)
    if st[-1] and k <= 16:
        r["ds", 0] = O.diag_scal_p(dp, st, p)
        r["ds", 1] = O.diag_scal_m(dm, st, p)
        for i in range(n + 1):
            r["pds", 0, i] = O.partial_diag_scal_p(dp, st, p, i)
            r["pds", 1, i] = O.partial_diag_scal_m(dm, st, p, i)
        for pf in (True, False):
            r["obs", pf] = np.nonzero(O.obs_states(k, st, pf) == 1.0)[0]
        for tr in (False, True):
            r["R", tr, "abs"] = O.R_i_inv_vec(lt, dp, dm, np.abs(x), st, k, tr)
            r["R", tr, "signed"] = O.R_i_inv_vec(lt, dp, dm, x, st, k, tr)
        r["xQy"] = O.x_partial_Q_y(lt, xg, yg, st)
        r["xDy"] = O.x_partial_D_y(dm, dp, st, xg, yg)
    _REFS[cid] = r
    return r


def single_refs(cid, k, lay):
    if cid in _REFS:
        return _REFS[cid]
    rng = _rng(cid)
    n, st = single_state(lay, k, _rng(f"single-{k}-{lay}"))
    from metmhn_amd import synthetic
    lt, dp, dm = synthetic.random_params(n, seed=zlib.crc32(cid.encode()) % 100000)
    V = 2 ** k
    p, x = rng.normal(size=V), rng.normal(size=V)
    xg, yg = rng.random(V) + 0.1, rng.random(V) + 0.1
    drv = rng.random(V) + 0.5
    r = {"in": (n, st, lt, dp, dm, p, x, xg, yg, drv)}
    ap = np.abs(p)
    r["kd"] = O.v_kron_diag(lt, st, np.ones(V))
    for tr in (False, True):
        off = O.v_kronvec(lt, ap, st, False, tr)
        r["m", False, tr] = off
        r["m", True, tr] = off + np.abs(r["kd"]) * ap
        for dg in (False, True):
            r["kv", dg, tr] = O.v_kronvec(lt, p, st, dg, tr)
    for dname, dr in (("one", 1.0), ("scalar", 0.7), ("vector", drv)):
        for tr in (False, True):
            r["R", dname, tr, "abs"] = O.v_R_inv_vec(lt, np.abs(x), st, dr, tr)
            r["R", dname, tr, "signed"] = O.v_R_inv_vec(lt, x, st, dr, tr)
    r["xQy"] = O.v_x_partial_Q_y(lt, xg, yg, st)
    if st[-1]:
        r["sd"] = O.v_scal_d_pt(dp, dm, st, p)
        for i in range(n + 1):
            r["dsd", i] = O.v_d_scal_d_pt(dp, dm, st, p, i)
        r["xDy"] = O.v_x_partial_D_y(dp, dm, st, xg, yg)
    _REFS[cid] = r
    return r


# ------------------------------------------------------------------------------------------------ engines
@pytest.fixture(scope="module")
def engines():
    """Engine(n, dtype) per (n, dtype, poison, solver); MMHN_POISON / MMHN_SOLVER are read when an engine is created."""
    from metmhn_amd import Engine
    cache = {}

    def get(n, dtype="f64", poison=False, solver=None):
        key = (n, dtype, poison, solver)
        if key not in cache:
            saved = {v: os.environ.get(v) for v in ("MMHN_POISON", "MMHN_SOLVER")}
            os.environ.pop("MMHN_POISON", None)
            os.environ.pop("MMHN_SOLVER", None)
            if poison:
                os.environ["MMHN_POISON"] = "1"
            if solver:
                os.environ["MMHN_SOLVER"] = solver
            try:
                cache[key] = Engine(n, dtype=dtype)
            finally:
                for v, val in saved.items():
                    if val is None:
                        os.environ.pop(v, None)
                    else:
                        os.environ[v] = val
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


# ------------------------------------------------------------------------------------------------ GPU sweep
@pytest.mark.gpu
@pytest.mark.parametrize("cid,k,lay,dtype,poison", _with_modes(_joint_cases()))
def test_joint_primitives_sweep(engines, cid, k, lay, dtype, poison):
    """kronvec (diag x transpose), kron_diag and - on seeded states - diag_scal, partial_diag_scal for every i,
    obs_states, resolvent (both transposes, both solvers), x_partial_Q_y, x_partial_D_y; on unseeded states the
    seeded-only calls must raise.  k = 18: kronvec and kron_diag only."""
    r = joint_refs(cid, k, lay)
    n, st, lt, dp, dm, p, x, xg, yg = r["in"]
    N = n + 1
    e = engines(n, dtype, poison)
    u = U[dtype]
    ck = Checker(f"[{cid} {dtype}{' poison' if poison else ''}]")
    tol = C_KV * (k + N) * u
    for tr in (False, True):
        for dg in (False, True):
            ck.bound(f"kronvec diag={dg:d} tr={tr:d}", e.kronvec(lt, p, st, dg, tr), r["kv", dg, tr], tol * r["m", dg, tr])
    ck.bound("kron_diag", e.kron_diag(lt, st), r["kd"], tol * np.abs(r["kd"]))
    if k > 16:
        return ck.done()
    if not st[-1]:
        ck.raises("diag_scal p on an unseeded state", lambda: e.diag_scal(dp, st, p, 0))
        ck.raises("diag_scal m on an unseeded state", lambda: e.diag_scal(dm, st, p, 1))
        ck.raises("partial_diag_scal on an unseeded state", lambda: e.partial_diag_scal(dp, st, p, 0, 0))
        ck.raises("obs_states on an unseeded state", lambda: e.obs_indices(st, True))
        return ck.done()
    for w, ld in ((0, dp), (1, dm)):
        ck.bound(f"diag_scal which={w}", e.diag_scal(ld, st, p, w), r["ds", w], tol * np.abs(r["ds", w]))
        for i in range(N):
            ref = r["pds", w, i]
            ck.bound(f"partial_diag_scal which={w} i={i}", e.partial_diag_scal(ld, st, p, i, w), ref, tol * np.abs(ref))
    for pf in (True, False):
        ck.exact(f"obs_states pt_first={pf}", e.obs_indices(st, pf), r["obs", pf])
    tol_r = C_R * (k + 1) * (k + N) * u
    for solver in (None, "jacobi"):
        es = engines(n, dtype, poison, solver)
        for tr in (False, True):
            ra = r["R", tr, "abs"]
            ck.bound(f"resolvent x>=0 tr={tr:d} solver={solver}", es.resolvent(lt, dp, dm, np.abs(x), st, tr), ra,
                     tol_r * ra)
            ck.bound(f"resolvent signed x tr={tr:d} solver={solver}", es.resolvent(lt, dp, dm, x, st, tr),
                     r["R", tr, "signed"], tol_r * ra)
    rt = RTOL_G[dtype]
    ck.rows("x_partial_Q_y", e.x_partial_Q_y(lt, xg, yg, st), r["xQy"], rt)
    a, b = e.x_partial_D_y(dp, dm, st, xg, yg)
    ck.rows("x_partial_D_y d_dp", a, r["xDy"][0], rt)
    ck.rows("x_partial_D_y d_dm", b, r["xDy"][1], rt)
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,k,lay,dtype,poison", _with_modes(_single_cases()))
def test_single_primitives_sweep(engines, cid, k, lay, dtype, poison):
    """v_kronvec (diag x transpose), v_kron_diag with and without the vector, v_resolvent (d_rates None / scalar != 1 /
    vector, both transposes, both solvers), v_x_partial_Q_y (G and d_diag); with the seeding event in the state also
    v_scal_d_pt, v_d_scal_d_pt for every i and v_x_partial_D_y, which must raise without it."""
    r = single_refs(cid, k, lay)
    n, st, lt, dp, dm, p, x, xg, yg, drv = r["in"]
    N = n + 1
    e = engines(n, dtype, poison)
    u = U[dtype]
    ck = Checker(f"[{cid} {dtype}{' poison' if poison else ''}]")
    tol = C_KV * (k + N) * u
    for tr in (False, True):
        for dg in (False, True):
            ck.bound(f"v_kronvec diag={dg:d} tr={tr:d}", e.v_kronvec(lt, p, st, dg, tr), r["kv", dg, tr],
                     tol * r["m", dg, tr])
    ck.bound("v_kron_diag", e.v_kron_diag(lt, st), r["kd"], tol * np.abs(r["kd"]))
    ck.bound("v_kron_diag with vector", e.v_kron_diag(lt, st, p), r["kd"] * p, tol * np.abs(r["kd"] * p))
    tol_r = C_R * (k + 1) * (k + N) * u
    for solver in (None, "jacobi"):
        es = engines(n, dtype, poison, solver)
        for dname, dr in (("none", None), ("scalar", 0.7), ("vector", drv)):
            rk = "one" if dr is None else dname
            for tr in (False, True):
                ra = r["R", rk, tr, "abs"]
                ck.bound(f"v_resolvent d_rates={dname} x>=0 tr={tr:d} solver={solver}",
                         es.v_resolvent(lt, np.abs(x), st, dr, tr), ra, tol_r * ra)
                ck.bound(f"v_resolvent d_rates={dname} signed x tr={tr:d} solver={solver}",
                         es.v_resolvent(lt, x, st, dr, tr), r["R", rk, tr, "signed"], tol_r * ra)
    rt = RTOL_G[dtype]
    G, dd = e.v_x_partial_Q_y(lt, xg, yg, st)
    Gr, ddr = r["xQy"]
    ck.rows("v_x_partial_Q_y G", G, Gr, rt)
    # d_diag[j] = -sum_{i != j} G[i, j]: each term within its row's bound
    rowtol = rt * (np.abs(Gr) + np.abs(Gr).max(axis=1, keepdims=True))
    ck.bound("v_x_partial_Q_y d_diag", dd, ddr, rowtol.sum(axis=0) - np.diagonal(rowtol))
    if not st[-1]:
        ck.raises("v_scal_d_pt without seeding", lambda: e.v_scal_d_pt(dp, dm, st, p))
        ck.raises("v_d_scal_d_pt without seeding", lambda: e.v_d_scal_d_pt(dp, dm, st, p, 0))
        ck.raises("v_x_partial_D_y without seeding", lambda: e.v_x_partial_D_y(dp, dm, st, xg, yg))
        return ck.done()
    a, b = e.v_scal_d_pt(dp, dm, st, p)
    ck.bound("v_scal_d_pt p", a, r["sd"][0], tol * np.abs(r["sd"][0]))
    ck.bound("v_scal_d_pt m", b, r["sd"][1], tol * np.abs(r["sd"][1]))
    for i in range(N):
        a, b = e.v_d_scal_d_pt(dp, dm, st, p, i)
        ra, rb = r["dsd", i]
        ck.bound(f"v_d_scal_d_pt p i={i}", a, ra, tol * np.abs(ra))
        ck.bound(f"v_d_scal_d_pt m i={i}", b, rb, tol * np.abs(rb))
    a, b = e.v_x_partial_D_y(dp, dm, st, xg, yg)
    ck.rows("v_x_partial_D_y d_dp", a, r["xDy"][0], rt)
    ck.rows("v_x_partial_D_y d_dm", b, r["xDy"][1], rt)
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize("kk", (14, 16))
def test_batched_kronvec_and_jacobi_step_unseeded(kk):
    """mmhn_kronvec_batched and the fused Jacobi step on an unseeded joint state past the tile bits: every tile goes down
    k_kv's seed = 0 branch.  y starts as NaNs on the device; against ref_kronvec (oracle/metmhn_ref.c) and
    lidg = 1 / (D_p + D_m - diag Q) of the dense definition (D_m = 0 without seeding), fp64 and fp32."""
    from oracle import cref
    from metmhn_amd import Engine, synthetic
    cref.load()
    n, st = joint_state("unseeded", kk, _rng(f"batched-unseeded-{kk}"))
    assert st[-1] == 0 and int(st.sum()) == kk
    lt, dp, dm = synthetic.random_params(n, seed=700 + kk)
    rng = np.random.default_rng(800 + kk)
    B = 2
    p = rng.random((B, 2 ** kk)) + 0.01
    rhs = rng.random((B, 2 ** kk))
    Dp, Dm = D.joint_D(dp, dm, st)
    kd = O.kron_diag(lt, st, kk)
    lidg = 1.0 / (Dp + Dm - kd)
    for dtype, u in (("f64", U["f64"]), ("f32", U["f32"])):
        with Engine(n, dtype=dtype) as e:
            tol = C_KV * (kk + n + 1) * u
            for tr in (False, True):
                for diag in (False, True):
                    y = e.kronvec_batched(lt, p, st, diag=diag, transpose=tr)
                    assert np.isfinite(y).all(), f"k={kk} {dtype} tr={tr} diag={diag}: unwritten states"
                    for b in range(B):
                        ref = cref.kronvec(lt, p[b], st, diag=diag, transpose=tr)
                        m = cref.kronvec(lt, p[b], st, diag=False, transpose=tr) + (np.abs(kd) * p[b] if diag else 0)
                        err = np.abs(y[b] - ref)
                        assert (err <= tol * m).all(), f"k={kk} {dtype} tr={tr} diag={diag} b={b}: {np.max(err / m)}"
                z = e.jacobi_step_batched(lt, dp, dm, p, rhs, st, transpose=tr)
                assert np.isfinite(z).all()
                for b in range(B):
                    q = cref.kronvec(lt, p[b], st, diag=False, transpose=tr)
                    ref = lidg * (q + rhs[b])
                    err = np.abs(z[b] - ref)
                    assert (err <= 2 * tol * ref).all(), f"jacobi k={kk} {dtype} tr={tr} b={b}: {np.max(err / ref)}"


@pytest.mark.gpu
def test_wrapper_argument_checks(engines):
    """Every single-vector wrapper checks its arguments before the C call (ValueError, nothing reaches the device), one
    bad argument at a time; the engine still gives the right answer on the next valid call."""
    n, st = joint_state("seeded", 5, _rng("args-joint"))
    from metmhn_amd import synthetic
    lt, dp, dm = synthetic.random_params(n, seed=5)
    e = engines(n)
    V = 2 ** 5
    rng = np.random.default_rng(3)
    p, x = rng.random(V), rng.random(V)
    ns, sst = single_state("seeded", 4, _rng("args-single"))
    es = engines(ns)
    lts, dps, dms = synthetic.random_params(ns, seed=6)
    Vs = 2 ** 4
    ps, xs = rng.random(Vs), rng.random(Vs)
    bad_lt = (lt[:-1, :-1], lt[:, :-1], lt.ravel())
    bad_d = (dp[:-1], np.append(dp, 0.0), dp[None, :])
    bad_st = (st[:-1], np.append(st, 0), st.astype(np.float64) * 0.5, np.where(st == 1, 2, 0), st[None, :])
    bad_vec = (p[:-1], np.append(p, 1.0), p[:V // 2], p[None, :])
    calls = {
        "kronvec": (lambda a: e.kronvec(*a), (lt, p, st)),
        "kron_diag": (lambda a: e.kron_diag(*a), (lt, st)),
        "diag_scal": (lambda a: e.diag_scal(*a, 0), (dp, st, p)),
        "resolvent": (lambda a: e.resolvent(*a), (lt, dp, dm, x, st)),
        "x_partial_Q_y": (lambda a: e.x_partial_Q_y(*a), (lt, x, p, st)),
        "x_partial_D_y": (lambda a: e.x_partial_D_y(*a), (dp, dm, st, x, p)),
        "partial_diag_scal": (lambda a: e.partial_diag_scal(*a, 0), (dp, st, p, 1)),
        "obs_indices": (lambda a: e.obs_indices(*a), (st, True)),
        "kronvec_batched": (lambda a: e.kronvec_batched(*a), (lt, p[None, :], st)),
        "jacobi_step_batched": (lambda a: e.jacobi_step_batched(*a), (lt, dp, dm, p[None, :], x[None, :], st)),
        "v_kronvec": (lambda a: es.v_kronvec(*a), (lts, ps, sst)),
        "v_resolvent": (lambda a: es.v_resolvent(*a), (lts, xs, sst, 0.7)),
        "v_x_partial_Q_y": (lambda a: es.v_x_partial_Q_y(*a), (lts, xs, ps, sst)),
        "v_kron_diag": (lambda a: es.v_kron_diag(*a), (lts, sst, ps)),
        "v_scal_d_pt": (lambda a: es.v_scal_d_pt(*a), (dps, dms, sst, ps)),
        "v_d_scal_d_pt": (lambda a: es.v_d_scal_d_pt(*a), (dps, dms, sst, ps, 1)),
        "v_x_partial_D_y": (lambda a: es.v_x_partial_D_y(*a), (dps, dms, sst, xs, ps)),
    }
    kinds = {"kronvec": "tvs", "kron_diag": "ts", "diag_scal": "dsv", "resolvent": "tddvs", "x_partial_Q_y": "tvvs",
             "x_partial_D_y": "ddsvv", "partial_diag_scal": "dsvi", "obs_indices": "s-", "kronvec_batched": "tbs",
             "jacobi_step_batched": "tddbbs", "v_kronvec": "tvs", "v_resolvent": "tvsr", "v_x_partial_Q_y": "tvvs",
             "v_kron_diag": "tsv", "v_scal_d_pt": "ddsv", "v_d_scal_d_pt": "ddsvi", "v_x_partial_D_y": "ddsvv"}
    checked = 0
    for name, (fn, args) in calls.items():
        single = name.startswith("v_")
        good = fn(args)                                          # valid call first
        for pos, kind in enumerate(kinds[name]):
            if kind == "t":
                bads = (lts[:-1, :-1], lts[:, :-1], lts.ravel()) if single else bad_lt
            elif kind == "d":
                bads = (dps[:-1], np.append(dps, 0.0), dps[None, :]) if single else bad_d
            elif kind == "s":
                bads = ((sst[:-1], np.append(sst, 0), sst.astype(np.float64) * 0.5, np.where(sst == 1, 2, 0),
                         sst[None, :]) if single else bad_st)
            elif kind == "v":
                bads = (ps[:-1], np.append(ps, 1.0), ps[:Vs // 2], ps[None, :]) if single else bad_vec
            elif kind == "b":
                bads = (p[None, :-1], p[None, :V // 2])
            elif kind == "i":
                bads = (-1, (ns if single else n) + 1, 1.0, True)
            elif kind == "r":
                bads = (np.ones(Vs - 1), np.ones(Vs + 1), np.ones((1, Vs)))
            else:
                continue
            for bad in bads:
                a = list(args)
                a[pos] = bad
                with pytest.raises(ValueError):
                    fn(tuple(a))
                checked += 1
        again = fn(args)                                         # the engine is unharmed
        for g, h in zip(good if isinstance(good, tuple) else (good,), again if isinstance(again, tuple) else (again,)):
            np.testing.assert_allclose(h, g, rtol=1e-12, atol=1e-14 * np.abs(g).max(), err_msg=name)
    assert checked > 150
    # and the values are right: the k = 5 seeded state against the oracle after all the refused calls
    np.testing.assert_allclose(e.kronvec(lt, p, st), O.kronvec(lt, p, st), rtol=1e-12, atol=0)
    np.testing.assert_allclose(e.resolvent(lt, dp, dm, x, st), O.R_i_inv_vec(lt, dp, dm, x, st, 5), rtol=1e-12, atol=0)
    np.testing.assert_allclose(es.v_resolvent(lts, xs, sst, 0.7), O.v_R_inv_vec(lts, xs, sst, 0.7), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ CPU: oracle vs dense
def _lower_solve(M, b, transpose):
    """(M or M^T)^-1 b for a lower-triangular M (states only move to supersets: Q[to, from] has to > from), in the
    dtype of M."""
    if transpose:
        M = M.T
    V = b.shape[0]
    y = np.zeros(V, dtype=M.dtype)
    order = range(V - 1, -1, -1) if transpose else range(V)
    for i in order:
        y[i] = (b[i] - M[i, :] @ y) / M[i, i]
    return y


def _cstep(f, base, idx, h=LD("1e-40")):
    """Complex-step derivative of f at base along the entry idx, in long double."""
    z = np.asarray(base, dtype=np.clongdouble).copy()
    z[idx] += 1j * h
    return (np.imag(f(z)) / h).astype(LD)


DENSE_JOINT = [("k0", "unseeded", 0), ("seed-only", "seeded", 1), ("pair-unseeded", "paired", 2),
               ("unseeded-k5", "unseeded", 5), ("unseeded-k7", "unseeded", 7), ("pt_seed-k5", "pt_seed", 5),
               ("mt_seed-k5", "mt_seed", 5), ("pt_seed-k2", "pt_seed", 2), ("mt_seed-k2", "mt_seed", 2),
               ("seeded-k7", "seeded", 7), ("paired-k7", "paired", 7), ("lone-k6", "lone", 6)]


@pytest.mark.parametrize("tag,lay,k", DENSE_JOINT, ids=[c[0] for c in DENSE_JOINT])
def test_oracle_joint_primitives_against_dense_longdouble(tag, lay, k):
    """oracle/metmhn_oracle.py's joint primitives against the generator built entry by entry from the transition rules
    (oracle/dense.py) in long double, at the states the golden vectors lack; derivatives by complex steps."""
    from metmhn_amd import synthetic
    n, st = joint_state(lay, k, _rng(f"dense-{tag}"))
    N, V, u = n + 1, 2 ** k, U["f64"]
    lt, dp, dm = synthetic.random_params(n, seed=zlib.crc32(tag.encode()) % 1000)
    rng = _rng(f"dense-vec-{tag}")
    p, x = rng.normal(size=V), rng.normal(size=V)
    ck = Checker(f"[dense {tag}]")
    Q = D.joint_Q(lt, st, LD)
    dq = np.diagonal(Q).copy()
    Qoff = Q - np.diag(dq)
    tol = C_KV * (k + N) * u
    pl = p.astype(LD)
    for tr in (False, True):
        Qt, Qo = (Q.T, Qoff.T) if tr else (Q, Qoff)
        for dg in (False, True):
            ref = (Qt if dg else Qo) @ pl
            m = Qo @ np.abs(pl) + (np.abs(dq) * np.abs(pl) if dg else 0)
            ck.bound(f"kronvec diag={dg:d} tr={tr:d}", O.kronvec(lt, p, st, dg, tr), ref, tol * m)
    ck.bound("kron_diag", O.kron_diag(lt, st, k), dq, tol * np.abs(dq))
    if st[-1]:
        Dp, Dm = D.joint_D(dp, dm, st, LD)
        ck.bound("diag_scal_p", O.diag_scal_p(dp, st, p), Dp * pl, tol * np.abs(Dp * pl))
        ck.bound("diag_scal_m", O.diag_scal_m(dm, st, p), Dm * pl, tol * np.abs(Dm * pl))
        for i in range(N):
            dDp = _cstep(lambda z: D.joint_D(z, dm, st, np.clongdouble)[0], dp, i)
            dDm = _cstep(lambda z: D.joint_D(dp, z, st, np.clongdouble)[1], dm, i)
            ck.bound(f"partial_diag_scal_p i={i}", O.partial_diag_scal_p(dp, st, p, i), dDp * pl, tol * np.abs(dDp * pl))
            ck.bound(f"partial_diag_scal_m i={i}", O.partial_diag_scal_m(dm, st, p, i), dDm * pl, tol * np.abs(dDm * pl))
        slots = D._slots(st)
        maskP = sum(1 << b for b, (e_, t) in enumerate(slots) if t == 0)
        maskM = sum(1 << b for b, (e_, t) in enumerate(slots) if t == 1)
        seedb = 1 << (k - 1)
        for pf, mask in ((True, maskP), (False, maskM)):
            want = [s for s in range(V) if (s & mask) == mask and s & seedb]
            ck.exact(f"obs_states pt_first={pf}", np.nonzero(O.obs_states(k, st, pf) == 1.0)[0], want)
        M = np.diag(Dp + Dm) - Q
        tol_r = C_R * (k + 1) * (k + N) * u
        for tr in (False, True):
            ra = _lower_solve(M, np.abs(x).astype(LD), tr)
            ck.bound(f"R_i_inv_vec x>=0 tr={tr:d}", O.R_i_inv_vec(lt, dp, dm, np.abs(x), st, k, tr), ra, tol_r * ra)
            ck.bound(f"R_i_inv_vec signed tr={tr:d}", O.R_i_inv_vec(lt, dp, dm, x, st, k, tr),
                     _lower_solve(M, x.astype(LD), tr), tol_r * ra)
        if k <= 7:
            xg, yg = rng.random(V) + 0.1, rng.random(V) + 0.1
            xl, yl = xg.astype(LD), yg.astype(LD)
            G = np.zeros((N, N), dtype=LD)
            for i in range(N):
                for j in range(N):
                    G[i, j] = _cstep(lambda z: xl @ (D.joint_Q(z, st, np.clongdouble) @ yl), lt, (i, j))
            ck.rows("x_partial_Q_y", O.x_partial_Q_y(lt, xg, yg, st), G, RTOL_G["f64"])
            gp = np.array([_cstep(lambda z: xl @ (D.joint_D(z, dm, st, np.clongdouble)[0] * yl), dp, i) for i in range(N)])
            gm = np.array([_cstep(lambda z: xl @ (D.joint_D(dp, z, st, np.clongdouble)[1] * yl), dm, i) for i in range(N)])
            a, b = O.x_partial_D_y(dm, dp, st, xg, yg)
            ck.rows("x_partial_D_y d_dp", a, gp, RTOL_G["f64"])
            ck.rows("x_partial_D_y d_dm", b, gm, RTOL_G["f64"])
    ck.done()


DENSE_SINGLE = [("k0", "unseeded", 0), ("seed-only", "seeded", 1), ("unseeded-k4", "unseeded", 4),
                ("seeded-k6", "seeded", 6)]


@pytest.mark.parametrize("tag,lay,k", DENSE_SINGLE, ids=[c[0] for c in DENSE_SINGLE])
def test_oracle_single_primitives_against_dense_longdouble(tag, lay, k):
    """The oracle's single-tumour primitives against oracle/dense.py's single_Q / single_D in long double."""
    from metmhn_amd import synthetic
    n, st = single_state(lay, k, _rng(f"dense-single-{tag}"))
    N, V, u = n + 1, 2 ** k, U["f64"]
    lt, dp, dm = synthetic.random_params(n, seed=zlib.crc32(tag.encode()) % 1000)
    rng = _rng(f"dense-single-vec-{tag}")
    p, x = rng.normal(size=V), rng.normal(size=V)
    drv = rng.random(V) + 0.5
    ck = Checker(f"[dense single {tag}]")
    Q = D.single_Q(np.exp(lt.astype(LD)), st)
    dq = np.diagonal(Q).copy()
    Qoff = Q - np.diag(dq)
    tol = C_KV * (k + N) * u
    pl = p.astype(LD)
    for tr in (False, True):
        Qt, Qo = (Q.T, Qoff.T) if tr else (Q, Qoff)
        for dg in (False, True):
            m = Qo @ np.abs(pl) + (np.abs(dq) * np.abs(pl) if dg else 0)
            ck.bound(f"v_kronvec diag={dg:d} tr={tr:d}", O.v_kronvec(lt, p, st, dg, tr), (Qt if dg else Qo) @ pl, tol * m)
    ck.bound("v_kron_diag", O.v_kron_diag(lt, st, np.ones(V)), dq, tol * np.abs(dq))
    tol_r = C_R * (k + 1) * (k + N) * u
    for dname, dr in (("one", 1.0), ("scalar", 0.7), ("vector", drv)):
        M = np.diag(np.broadcast_to(np.asarray(dr, dtype=LD), (V,))) - Q
        for tr in (False, True):
            ra = _lower_solve(M, np.abs(x).astype(LD), tr)
            ck.bound(f"v_R_inv_vec {dname} x>=0 tr={tr:d}", O.v_R_inv_vec(lt, np.abs(x), st, dr, tr), ra, tol_r * ra)
            ck.bound(f"v_R_inv_vec {dname} signed tr={tr:d}", O.v_R_inv_vec(lt, x, st, dr, tr),
                     _lower_solve(M, x.astype(LD), tr), tol_r * ra)
    xg, yg = rng.random(V) + 0.1, rng.random(V) + 0.1
    xl, yl = xg.astype(LD), yg.astype(LD)
    G = np.zeros((N, N), dtype=LD)
    for i in range(N):
        for j in range(N):
            G[i, j] = _cstep(lambda z: xl @ (D.single_Q(np.exp(z), st) @ yl), lt, (i, j))
    Go, ddo = O.v_x_partial_Q_y(lt, xg, yg, st)
    ck.rows("v_x_partial_Q_y G", Go, G, RTOL_G["f64"])
    ck.rows("v_x_partial_Q_y d_diag", ddo, -G.sum(axis=0) + np.diagonal(G), RTOL_G["f64"])
    if st[-1]:
        seeded = (np.arange(V) >> (k - 1)) & 1

        def scal(ldp, ldm):
            a = D.single_D(np.exp(np.append(ldp[:n], 0.0)), st) * (1 - seeded)
            b = D.single_D(np.exp(ldm), st) * seeded
            return a, b
        a, b = scal(dp.astype(LD), dm.astype(LD))
        ao, bo = O.v_scal_d_pt(dp, dm, st, p)
        ck.bound("v_scal_d_pt p", ao, a * pl, tol * np.abs(a * pl))
        ck.bound("v_scal_d_pt m", bo, b * pl, tol * np.abs(b * pl))
        for i in range(N):
            da = _cstep(lambda z: scal(z, dm.astype(np.clongdouble))[0], dp, i)
            db = _cstep(lambda z: scal(dp.astype(np.clongdouble), z)[1], dm, i)
            ao, bo = O.v_d_scal_d_pt(dp, dm, st, p, i)
            ck.bound(f"v_d_scal_d_pt p i={i}", ao, da * pl, tol * np.abs(da * pl))
            ck.bound(f"v_d_scal_d_pt m i={i}", bo, db * pl, tol * np.abs(db * pl))
        gp = np.array([xl @ (_cstep(lambda z: scal(z, dm.astype(np.clongdouble))[0], dp, i) * yl) for i in range(N)])
        gm = np.array([xl @ (_cstep(lambda z: scal(dp.astype(np.clongdouble), z)[1], dm, i) * yl) for i in range(N)])
        a, b = O.v_x_partial_D_y(dp, dm, st, xg, yg)
        ck.rows("v_x_partial_D_y d_dp", a, gp, RTOL_G["f64"])
        ck.rows("v_x_partial_D_y d_dm", b, gm, RTOL_G["f64"])
    ck.done()


def test_sweep_covers_the_tile_boundary():
    """The GPU sweep's shapes: both sides of the tile bits, every joint layout past them, an event slot and the seeding
    slot at or above bit TB in one case, unseeded joint states, fp32 at k in FP32_K, half of the cases poisoned and the
    dead-tile case among them."""
    joint = _joint_cases()
    ks = {k for _, k, _ in joint}
    assert {0, 1, 2, 11, 12, 13, 14, 16, 18} <= ks
    for k in (13, 14, 16):
        assert {lay for _, kk, lay in joint if kk == k and lay != "top"} == set(JOINT_LAYOUTS_LARGE)
    # n = 31: the last slots and the seeding slot 62 of a joint state, the events 29 - 31 of a single-tumour state, fp64 and fp32
    for cases, state, last in ((joint, joint_state, [56, 57, 58, 59, 60, 61, 62]), (_single_cases(), single_state, [29, 30, 31])):
        top = [c for c in cases if c[2] == "top"]
        assert len(top) == 1 and top[0][1] == 13 > TB and 13 in FP32_K
        n, st = state("top", 13, None)
        assert n == 31 and int(st.sum()) == 13 and st[last].all() and len(st) == last[-1] + 1
    n, st = joint_state("lone", 14, _rng("joint-14-lone"))
    slots = D._slots(st)
    assert slots[-1][1] == 2 and len(slots) - 1 >= TB and slots[TB][1] != 2
    assert {k for _, k, _ in _single_cases()} == {0, 1, 5, 11, 12, 13, 14, 16}
    modes = [p.values for p in _with_modes(joint) + _with_modes(_single_cases())]
    assert sum(m[4] for m in modes) * 2 >= len(modes)
    assert {m[1] for m in modes if m[3] == "f32"} == set(FP32_K)
    assert any(m[0] == "joint-k14-lone" and m[4] for m in modes)
