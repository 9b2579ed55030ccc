"""Drop-in for metmhn/regularized_optimization.py (same names, arguments, return values).

`score`, `score_and_grad`, `score_reg`, `score_and_grad_reg`, `learn_mhn` and the penalties
keep the reference signatures (regularized_optimization.py:11-334); the per-patient work
(metmhn/jx/*) runs on the GPU through the C ABI.  The cohort is uploaded and laid out once
per distinct `dat` (cached), parameters go up and a 484-double result comes back per call.
With an initialised torch.distributed process group every rank evaluates its own patient
shard and one all-reduce combines the partial sums (metmhn_amd.distributed).
"""
from __future__ import annotations

import zlib
from typing import Callable

import numpy as np
import scipy.optimize as opt

from . import distributed as _dist
from .engine import Engine

_CACHE: dict = {}
_MAX_CACHE = 4
_OPTIONS = {"device": None, "dtype": "f64", "shard": True, "strict_guard": False}


def configure(device: int | None = None, dtype: str = "f64", shard: bool = True, strict_guard: bool = False):
    """Pick the GPU (default: LOCAL_RANK or 0), the engine dtype and whether to shard over ranks.
    strict_guard: the cache guard hashes ALL of `dat` on every call (the reference is a pure function of `dat`);
    default: all of it up to 256 KB, 64 sampled rows above that."""
    from .engine import set_default_device
    _OPTIONS.update(device=device, dtype=dtype, shard=shard, strict_guard=bool(strict_guard))
    set_default_device(device)
    invalidate()


def invalidate(dat=None):
    """Drop the cached device cohort of `dat` (all of them if None).  The cache recognises an array by identity
    (object, buffer address, shape) plus a CRC of 64 sampled rows (`_sample_crc`): in-place edits that touch the
    sampled rows are noticed and re-uploaded, for anything finer call this after changing a cohort array IN PLACE."""
    for key in list(_CACHE):
        if dat is None or key[0] == id(dat):
            _CACHE.pop(key)[0].close()


def _rank_world():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return 0, 1


def _join_comm(eng: Engine, rank: int, world: int) -> bool:
    """Attach the engine to an RCCL communicator over the ranks of the torch.distributed job (backend nccl): the
    id travels through torch's object broadcast, the all-reduce itself then runs inside mmhn_cohort_sums on the
    engine's stream.  False -> the caller keeps the host-staged torch all-reduce (gloo / CPU tests).

    The decision is COLLECTIVE: rank 0 always broadcasts (a failure sentinel if it could not make an id), every rank
    reports whether its mmhn_comm_init succeeded, and the device communicator is used only if all did - otherwise
    every rank destroys its half and all of them use torch's collective (no rank is ever left alone in one of the two).
    MMHN_COMM_TIMEOUT (seconds, default 180): a rank whose ncclCommInitRank does not return fails instead of hanging."""
    import os
    import torch.distributed as dist
    from .engine import unique_id
    if world > 1 and dist.get_backend() != "nccl":
        return False
    strict = os.environ.get("MMHN_STRICT_COMM") == "1"
    err = None
    box = [None]
    if rank == 0:
        try:
            box[0] = unique_id()
        except Exception as exc:
            err = exc
    if world > 1:
        dist.broadcast_object_list(box, src=0)                # always entered by every rank
    if box[0] is None:
        all_ok, msg = False, f"rank 0 could not create an RCCL id ({err})"
    else:
        store = None
        if world > 1:
            from torch.distributed.distributed_c10d import _get_default_store
            store = _get_default_store()
        # (no collective in here: a rank that fails before ncclCommInitRank tells the others through the store, and a rank
        # still blocked in it gives up within a fraction of a second instead of after MMHN_COMM_TIMEOUT - distributed.py)
        all_ok, msg = _dist.collective_init(lambda: eng.comm_init(box[0], rank, world), rank, world, store,
                                            timeout=float(os.environ.get("MMHN_COMM_TIMEOUT", "180")))
    if all_ok:
        return True
    if getattr(eng, "comm_size", 1) > 1 or box[0] is not None:
        try:
            eng.comm_destroy()                                # some other rank failed: nobody uses the device communicator
        except Exception:                                     # noqa: BLE001
            pass
    if strict:
        raise RuntimeError(f"metmhn_amd: in-library RCCL communicator unavailable on some rank ({msg})")
    import warnings
    warnings.warn(f"metmhn_amd: in-library RCCL communicator unavailable ({msg}); using torch.distributed")
    return False


def _cache_key(dat, rank, world):
    """Identity key of a cohort array (no pass over its bytes on the per-evaluation path)."""
    if isinstance(dat, np.ndarray):
        return (id(dat), dat.__array_interface__["data"][0], dat.shape, dat.dtype.str, rank, world, _OPTIONS["dtype"])
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))          # lists, foreign array types: by content
    return (None, zlib.crc32(arr.tobytes()), arr.shape, "i1", rank, world, _OPTIONS["dtype"])


_CRC_ROWS = {}


def _digest(arr: np.ndarray) -> int:
    """64-bit digest of a contiguous array: xxh3 where the package is there (13 us for the 208 KB of the LUAD-reduced
    cohort - zlib's CRC takes 240 us, longer than a score-only evaluation of that cohort), else zlib.crc32."""
    if arr.size == 0:
        return 0
    flat = arr.reshape(-1).view(np.uint8)                     # (memoryview.cast refuses shapes with a zero in them)
    try:
        import xxhash                                         # optional: `pip install metmhn_amd[fast]`
    except ImportError:
        return zlib.crc32(flat)
    return xxhash.xxh3_64_intdigest(flat)


def _sample_crc(dat: np.ndarray) -> int:
    """Guard of the identity-keyed cache against in-place edits, run while the GPU evaluates: the CRC of the whole array
    up to 256 KB (every LUAD-sized cohort: ~50 us) or with configure(strict_guard=True); of 64 evenly spaced rows above
    that (a full pass over a large cohort per evaluation would be host time on the critical path) - there a single
    edited row between the samples still needs invalidate()."""
    if dat.shape[0] <= 64 or dat.nbytes <= (256 << 10) or _OPTIONS["strict_guard"]:
        return _digest(np.ascontiguousarray(dat))
    idx = _CRC_ROWS.get(dat.shape[0])
    if idx is None:
        if len(_CRC_ROWS) > 64:
            _CRC_ROWS.clear()
        idx = _CRC_ROWS[dat.shape[0]] = np.linspace(0, dat.shape[0] - 1, 64).astype(np.int64)
    return _digest(np.ascontiguousarray(dat[idx]))


def _engine_for(dat, check: bool = True) -> Engine:
    """The engine holding `dat`'s layout.  check=False: a cache hit is returned without the in-place-edit guard - the
    caller runs it next to the GPU (_result(..., guard=dat)) and evaluates again if it fires."""
    import os
    import weakref
    rank, world = _rank_world()
    if not _OPTIONS["shard"]:
        rank, world = 0, 1
    key = _cache_key(dat, rank, world)
    hit = _CACHE.get(key)
    if hit is not None and (hit[1] is None or hit[1]() is dat):
        if not check or not isinstance(dat, np.ndarray) or not _stale_anywhere(hit[0], dat, world):
            return hit[0]
        # same array object, edited in place: the SAME engine (callers may hold it; its communicator stays) gets the new rows
        _load_rows(hit[0], dat, rank, world, weights=hit[0]._weights, groups=hit[0]._groups)
        return hit[0]
    if hit is not None:                                       # the id was recycled for another array
        _CACHE.pop(key)[0].close()
    for k2 in [k2 for k2, (e2, r2) in _CACHE.items() if r2 is not None and r2() is None]:
        _CACHE.pop(k2)[0].close()                             # cohorts whose array is gone free their HBM now
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    if len(_CACHE) >= _MAX_CACHE:
        _CACHE.pop(next(iter(_CACHE)))[0].close()
    n_mut = (arr.shape[1] - 3) // 2
    eng = Engine(n_mut, device=_OPTIONS["device"], dtype=_OPTIONS["dtype"])
    _load_rows(eng, dat, rank, world, arr)
    # MMHN_FORCE_ALLREDUCE=1: run the collective even with one rank (exercises the RCCL path on a 1-GPU box)
    eng.world_size_hint = world
    eng._sharded = world > 1 or os.environ.get("MMHN_FORCE_ALLREDUCE") == "1"
    eng._device_comm = eng._sharded and _reduce_mode() != "host_fixed_order" and _join_comm(eng, rank, world)
    ref = None
    if isinstance(dat, np.ndarray):
        try:
            ref = weakref.ref(dat)
        except TypeError:
            ref = None
    _CACHE[key] = (eng, ref)
    return eng


def _check_weights(weights, n_rows: int):
    """float64 copy of `weights` [n_rows] (one per row of `dat`), or None."""
    if weights is None:
        return None
    w = np.array(weights, dtype=np.float64, copy=True)
    if w.shape != (n_rows,):
        raise ValueError(f"weights must have shape ({n_rows},): one per row of dat, got {w.shape}")
    return w


def _global_counts(arr: np.ndarray, weights=None):
    """(n_em, n_pat, n_unknown) over the WHOLE `dat` (every rank holds it): the weight of :121-128 is known without
    communication.  n_nm = n_pat - n_em - the rows of type 4, which have weight 1 of their own.  With row weights: the three
    weighted sums (a row of weight 0 counts as absent)."""
    if weights is None:
        return (float(arr[:, -3].sum()), float(arr.shape[0]), float(np.count_nonzero(arr[:, -1] == 4)))
    w = np.asarray(weights, dtype=np.float64)
    return (float(w[arr[:, -3] == 1].sum()), float(w.sum()), float(w[arr[:, -1] == 4].sum()))


def _shard_weights(weights: np.ndarray, arr: np.ndarray, rank: int, world: int) -> np.ndarray:
    """The weights of this rank's rows: sliced with the same indices as the rows themselves."""
    return weights if world == 1 else weights[_dist.shard_rows(arr, world)[rank]]


def _load_rows(eng: Engine, dat, rank: int, world: int, arr=None, weights=None, groups=None):
    """(Re)build the device layout of this rank's shard of `dat` on `eng`; weights (optional): one per row of `dat`;
    groups (optional): the (ptr, idx, w) the engine held (_set_groups)."""
    if arr is None:
        arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    rows = arr if world == 1 else arr[_dist.shard_rows(arr, world)[rank]]
    eng.set_cohort(rows)
    eng._weights = None                                       # (set_cohort cleared them)
    eng._groups = None                                        # (and the groups)
    eng._global_counts = _global_counts(arr)
    eng._sample_crc = _sample_crc(dat) if isinstance(dat, np.ndarray) else None
    if weights is not None:
        _set_weights(eng, arr, weights, rank, world)
    if groups is not None:
        _set_groups(eng, arr, groups, world)


def _set_weights(eng: Engine, arr: np.ndarray, weights, rank: int, world: int):
    """Give the engine that holds `arr`'s layout the row weights `weights` (None: remove them): one upload, no re-plan."""
    eng.set_row_weights(None if weights is None else _shard_weights(weights, arr, rank, world))
    eng._weights = None if weights is None else np.array(weights, dtype=np.float64, copy=True)
    eng._global_counts = _global_counts(arr, weights)


def _group_arrays(groups, n_rows: int):
    """(ptr, idx, w) of a RowGroups (Utilityfunctions.expand_missing) over a cohort of n_rows rows, checked for shape."""
    ptr = np.ascontiguousarray(np.asarray(groups.ptr, dtype=np.int64))
    idx = np.ascontiguousarray(np.asarray(groups.idx, dtype=np.int64))
    w = np.array(groups.weights, dtype=np.float64, copy=True)
    if ptr.ndim != 1 or ptr.shape[0] < 2 or idx.ndim != 1 or w.shape != (ptr.shape[0] - 1,) or int(ptr[-1]) != idx.shape[0]:
        raise ValueError(f"groups: ptr {ptr.shape}, idx {idx.shape} and weights {w.shape} do not describe group lists")
    if idx.size and (idx.min() < 0 or idx.max() >= n_rows):
        raise ValueError(f"groups: an index outside the {n_rows} rows of dat (dat must be groups.rows)")
    return ptr, idx, w


def _group_counts(arr: np.ndarray, ptr, idx, w):
    """(n_em, n_pat, n_unknown) with row groups: the group-weighted counts, a group taking seeding and type of its rows."""
    first = idx[ptr[:-1]]
    return (float(w[arr[first, -3] == 1].sum()), float(w.sum()), float(w[arr[first, -1] == 4].sum()))


def _set_groups(eng: Engine, arr: np.ndarray, groups, world: int):
    """Give the engine that holds `arr`'s layout the row groups (ptr, idx, w) (None: remove them): no re-plan."""
    if groups is None:
        eng.set_row_groups(None, None)
        eng._groups = None
        eng._global_counts = _global_counts(arr)
        return
    if world > 1:
        raise ValueError("metmhn_amd: groups= with configure(shard=True) and more than one rank: sharding cuts through "
                         "groups, row groups are evaluated on one rank")
    ptr, idx, w = groups
    eng.set_row_groups(ptr, idx, w)
    eng._groups = (ptr, idx, w)
    eng._global_counts = _group_counts(arr, ptr, idx, w)


def _weighted_engine(dat, weights, groups=None) -> Engine:
    """_engine_for(dat, check=False) holding `weights` (one per row of `dat`, or None) or the row groups `groups` (a
    RowGroups over `dat`, or None).  The engine keeps a copy of what it was given; when the call's differ they are
    uploaded and the global counts recomputed - the plan stays."""
    if groups is not None and weights is not None:
        raise ValueError("groups= and weights= exclude each other: the group weights (groups.weights) take the role of the row weights")
    eng = _engine_for(dat, check=False)
    if groups is not None or eng._groups is not None:
        rank, world = _rank_world() if _OPTIONS["shard"] else (0, 1)
        arr = np.asarray(dat)
        if groups is None:
            _set_groups(eng, arr, None, world)
        else:
            new = _group_arrays(groups, arr.shape[0])
            if eng._groups is None or not all(np.array_equal(a, b) for a, b in zip(new, eng._groups)):
                if eng._weights is not None:
                    _set_weights(eng, arr, None, rank, world)
                _set_groups(eng, arr, new, world)
            return eng
    held = eng._weights
    if weights is None and held is None:
        return eng
    w = _check_weights(weights, np.shape(dat)[0])
    if w is None or held is None or not np.array_equal(w, held):
        rank, world = _rank_world() if _OPTIONS["shard"] else (0, 1)
        _set_weights(eng, np.asarray(dat), w, rank, world)
    return eng


def _stale_anywhere(eng: Engine, dat, world: int) -> bool:
    """Has `dat` been edited in place since `eng` laid it out - on ANY rank (the ranks must decide together: a rebuild
    and the repeated evaluation are collective)?  Used where an engine is fetched outside an evaluation; inside one the bit
    rides in the evaluation's own all-reduce (_result)."""
    stale = isinstance(dat, np.ndarray) and eng._sample_crc != _sample_crc(dat)
    if world > 1:
        import torch
        import torch.distributed as dist
        flag = torch.tensor([1 if stale else 0], dtype=torch.int32, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        stale = bool(int(flag.item()))
    return stale


def _reduce_mode():
    import os
    return os.environ.get("MMHN_REDUCE", "")


def _result(eng: Engine, log_theta, log_d_p, log_d_m, perc_met: float, with_grad: bool, meanwhile: Callable = None,
            guard=None):
    """((score, d_theta, d_dp, d_dm), meanwhile's result).  EM and NM sums are combined on the device (the weight of
    regularized_optimization.py:121-128 only needs the global counts, known when the cohort is set): 1 + N^2 + 2N
    doubles come back - and, with several ranks, cross them in ONE all-reduce, inside the library on the engine's
    stream (RCCL) when the communicator is attached, else through torch.distributed.
    `meanwhile()` (host work that does not need the result: the penalty terms) runs while the GPU evaluates, and so
    does the cache guard of `guard` (the caller's `dat`, engine from _engine_for(dat, check=False)): if the array was
    edited in place since its layout was built, the result is dropped and the evaluation repeated on a fresh layout."""
    n_em, n_pat, n_unknown = eng._global_counts
    w, n_full = _dist.em_weight(n_em, n_pat, perc_met, n_unknown)
    guarded = isinstance(guard, np.ndarray)                   # (anything else was keyed by content: cannot be stale)
    many = eng._sharded and eng.world_size_hint > 1
    stale = False
    if many and guarded:
        # several ranks must decide TOGETHER whether to rebuild: the bit rides in the evaluation's own all-reduce (one
        # collective per evaluation), so the guard runs before the launch here (13 us on a LUAD-sized array)
        stale = eng._sample_crc != _sample_crc(guard)
    eng.cohort_wsums_begin(log_theta, log_d_p, log_d_m, w, with_grad=with_grad, flag=(1.0 if stale else 0.0) if many and guarded else None)
    try:
        if not many:
            stale = guarded and eng._sample_crc != _sample_crc(guard)          # one rank: next to the GPU
        aside = meanwhile() if meanwhile is not None and not stale else None
    finally:
        ws = eng.cohort_wsums_end()
    if eng._sharded and not eng._device_comm:
        ext = np.append(ws, 1.0 if (stale and many and guarded) else 0.0)       # (the same bit through torch's collective)
        ext = _dist.allreduce_sums_fixed_order(ext) if _reduce_mode() == "host_fixed_order" else _dist.allreduce_sums(ext)
        ws, stale_any = ext[:-1], ext[-1] > 0
    else:
        stale_any = eng.reduce_flag > 0
    if many and guarded:
        stale = bool(stale_any)
    if stale:
        rank, world = _rank_world() if _OPTIONS["shard"] else (0, 1)
        _load_rows(eng, guard, rank, world, weights=eng._weights, groups=eng._groups)   # the same engine (and communicator), the new rows, the weights / groups again
        return _result(eng, log_theta, log_d_p, log_d_m, perc_met, with_grad, meanwhile)
    if aside is None and meanwhile is not None:
        aside = meanwhile()
    return _dist.split_wsums(ws, eng.N, n_full), aside


# ---- penalties (host NumPy, as in the reference; regularized_optimization.py:11-52) ----

def L1(theta, eps: float = 1e-05):
    t = np.array(theta, dtype=np.float64, copy=True)
    if t.ndim == 2:
        np.fill_diagonal(t, 0.0)
    return np.sum(np.sqrt(t ** 2 + eps))


def L1_(theta, eps: float = 1e-05):
    t = np.array(theta, dtype=np.float64, copy=True)
    if t.ndim == 2:
        np.fill_diagonal(t, 0.0)
    return t.flatten() / np.sqrt(t.flatten() ** 2 + eps)


def sym_penal(log_theta, eps: float = 1e-05):
    t = np.array(log_theta, dtype=np.float64, copy=True)
    n = t.shape[0]
    np.fill_diagonal(t, 0.0)
    return 0.5 * (np.sum(np.sqrt(t ** 2 + t.T ** 2 - t * t.T + eps)) - n * np.sqrt(eps))


def sym_penal_(log_theta, eps: float = 1e-05):
    t = np.array(log_theta, dtype=np.float64, copy=True)
    np.fill_diagonal(t, 0.0)
    return ((2 * t - t.T) / (2 * np.sqrt(t ** 2 + t.T ** 2 - t * t.T + eps))).flatten()


def symmetric_penal(params, n_total: int, eps=1e-05):
    params = np.asarray(params, dtype=np.float64)
    log_theta = params[0:n_total ** 2].reshape((n_total, n_total))
    log_d_p = params[n_total ** 2:n_total * (n_total + 1)]
    log_d_m = params[n_total * (n_total + 1):]
    penal = np.array(sym_penal(log_theta) + L1(log_d_p) + L1(log_d_m))
    penal_ = np.concatenate((sym_penal_(log_theta), L1_(log_d_p), L1_(log_d_m)))
    return penal, penal_


# ---- objective -------------------------------------------------------------------------

def score(log_theta, log_d_p, log_d_m, dat, perc_met: float, weights=None, groups=None):
    """Log-likelihood of the dataset (regularized_optimization.py:55-130).

    weights (keyword, here and in score_and_grad, score_reg, score_and_grad_reg, learn_mhn): one weight w_i >= 0 per row of
    `dat`, finite and not all zero.  The objective is then the one of the cohort in which row i occurs w_i times (every sum
    over the rows and the three counts n_em, n_pat, n_unknown weighted; a row of weight 0 counts as absent).  Changing the
    weights of a cached cohort costs one upload, not a new plan; rows of weight 0 are still solved.

    groups (keyword, same functions): a RowGroups from Utilityfunctions.expand_missing - rows with unobserved entries as
    mixtures over their completions; `dat` is then groups.rows.  Every patient (group) scores logsumexp of its completions'
    lp, the counts are the group-weighted ones.  groups and weights together are a ValueError; one rank only."""
    eng = _weighted_engine(dat, weights, groups)
    return _result(eng, log_theta, log_d_p, log_d_m, perc_met, False, guard=dat)[0][0]


def score_and_grad(log_theta, log_d_p, log_d_m, dat, perc_met: float, weights=None, groups=None):
    """(score, d_theta, d_d_p, d_d_m)  (regularized_optimization.py:163-267).  weights, groups: see score."""
    eng = _weighted_engine(dat, weights, groups)
    return _result(eng, log_theta, log_d_p, log_d_m, perc_met, True, guard=dat)[0]


def met_status_posterior(log_theta, log_d_p, log_d_m, dat):
    """P(the metastasis had been seeded | PT genotype) under the model, for every row of `dat` with a primary tumour of
    its own (types 0, 1 and 4): the row is scored as a tumour of unknown status (type 4) on a relabelled copy with the
    MT, seeding and order columns cleared.  NaN for the rows of types 2 and 3.  float64 [n_pat]."""
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    out = np.full(arr.shape[0], np.nan)
    pick = np.isin(arr[:, -1], (0, 1, 4))
    if not pick.any():
        return out
    rows = arr[pick].copy()
    rows[:, 1:-3:2] = 0
    rows[:, -3] = 0
    rows[:, -2] = 0
    rows[:, -1] = 4
    with Engine((arr.shape[1] - 3) // 2, device=_OPTIONS["device"], dtype=_OPTIONS["dtype"]) as eng:
        eng.set_cohort(rows)
        out[pick] = eng.patient_status(log_theta, log_d_p, log_d_m)[1]
    return out


def seeding_forecast(log_theta, log_d_p, log_d_m, dat, until: str = "observation", backend: str = "device"):
    """What lies ahead of the primary tumour of every row of `dat` that has one of its own (types 0, 1 and 4), given that it
    has not seeded yet: (forecasts, seeded).  forecasts: MetMHN.seeding_forecasts of the rows' PT genotypes
    dat[:, 0:2*n:2] with obs1 = log_d_p, a model.SeedingForecasts whose rows of types 2 and 3 are NaN throughout; seeded
    [n_pat]: met_status_posterior's probability that the seeding has ALREADY happened - the forecast is conditional on
    "not yet", so P(seeded by the next look) = seeded + (1 - seeded) p_seed."""
    from .model import MetMHN, SeedingForecasts
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    n = (arr.shape[1] - 3) // 2
    pick = np.isin(arr[:, -1], (0, 1, 4))
    shapes = {"p_seed": (), "time": (), "before": (n,), "with_seed": (n,), "n_before": (n + 1,), "next": (n + 1,)}
    out = {name: np.full((arr.shape[0],) + shape, np.nan) for name, shape in shapes.items()}
    if pick.any():
        got = MetMHN(log_theta, log_d_p, log_d_m).seeding_forecasts(arr[pick][:, 0:2 * n:2], until, backend)
        for name in shapes:
            out[name][pick] = getattr(got, name)
    return SeedingForecasts(**out), met_status_posterior(log_theta, log_d_p, log_d_m, dat)


def seeding_risk(log_theta, log_d_p, log_d_m, dat, until: str = "observation", backend: str = "device"):
    """The scalar answers of seeding_forecast for every row of `dat` with a primary tumour of its own (types 0, 1 and 4),
    from ONE backward sweep over all genotypes of the model instead of a lattice per distinct genotype: (risk, seeded).
    risk: a model.SeedingLandscape over the rows - p_seed, time, new_events, seed_events [n_pat] of the rows' PT genotypes
    dat[:, 0:2*n:2] with obs1 = log_d_p (MetMHN.seeding_landscape_at), NaN and code -1 for the rows of types 2 and 3;
    seeded [n_pat]: met_status_posterior's probability that the seeding has already happened, as seeding_forecast returns
    it."""
    from .model import MetMHN, SeedingLandscape
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    n = (arr.shape[1] - 3) // 2
    pick = np.isin(arr[:, -1], (0, 1, 4))
    out = {name: np.full(arr.shape[0], np.nan) for name in SeedingLandscape.FIELDS}
    codes = np.full(arr.shape[0], -1, dtype=np.int64)
    if pick.any():
        got = MetMHN(log_theta, log_d_p, log_d_m).seeding_landscape_at(arr[pick][:, 0:2 * n:2], until, backend)
        for name in SeedingLandscape.FIELDS:
            out[name][pick] = getattr(got, name)
        codes[pick] = got.codes
    return SeedingLandscape(**out, codes=codes), met_status_posterior(log_theta, log_d_p, log_d_m, dat)


def _stratum_table(strata, typ, codes, prob) -> dict:
    """{stratum: (codes, observed, expected)} of genotype_fit and metastasis_fit for the `strata` (name, row type) with rows."""
    table = {}
    for stratum, ty in strata:
        rows = typ == ty
        if rows.any():
            uniq, first, counts = np.unique(codes[rows], return_index=True, return_counts=True)
            table[stratum] = (uniq, counts.astype(np.int64), int(rows.sum()) * prob[rows][first])
    return table


def genotype_fit(log_theta, log_d_p, log_d_m, dat, backend: str = "device"):
    """How well the model's exact genotype distribution of the primary tumour fits the PT genotypes of `dat`, from ONE
    forward sweep over all genotypes (MetMHN.genotype_distribution_at with obs1 = log_d_p).  A namespace of
    prob [n_pat]: the probability of the row's PT genotype dat[:, 0:2*n:2] within its stratum - unseeded / mass[0] for a row
        of type 0 ("NM"), seeded / mass[1] for type 1 ("EM-PT"), unseeded + seeded for type 4 ("unknown"); NaN for types 2, 3;
    codes [n_pat]: the rows' genotype codes, -1 for types 2 and 3;
    table: {stratum: (codes, observed, expected)} for the strata with rows - the distinct genotype codes of the stratum's
        rows, ascending, how many rows carry each, and rows of the stratum x the genotype's probability within it;
    summary: the model.GenotypeSummary of the whole lattice;  residuals: summary.compare(dat)."""
    from types import SimpleNamespace
    from .model import GENOTYPE_STRATA, MetMHN
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    n = (arr.shape[1] - 3) // 2
    typ = arr[:, -1]
    pick = np.isin(typ, (0, 1, 4))
    got = MetMHN(log_theta, log_d_p, log_d_m).genotype_distribution_at(arr[pick][:, 0:2 * n:2], backend)
    mass = got.summary.mass
    within = {0: got.unseeded / mass[0], 1: got.seeded / mass[1], 4: got.total}
    prob = np.full(arr.shape[0], np.nan)
    codes = np.full(arr.shape[0], -1, dtype=np.int64)
    codes[pick] = got.codes
    t = typ[pick]
    prob[pick] = np.select([t == 0, t == 1], [within[0], within[1]], within[4])
    table = _stratum_table(zip(GENOTYPE_STRATA, (0, 1, 4)), typ, codes, prob)
    return SimpleNamespace(prob=prob, codes=codes, table=table, summary=got.summary, residuals=got.summary.compare(arr))


def metastasis_fit(log_theta, log_d_p, log_d_m, dat, backend: str = "device"):
    """How well the model's exact genotype distribution of the metastasis fits the MT genotypes of `dat`, from ONE forward
    sweep over all genotypes (MetMHN.metastasis_distribution_at with obs1 = log_d_p, obs2 = log_d_m) - genotype_fit's
    counterpart for the rows of types 2 ("EM-MT") and 3 ("paired").  A namespace of
    prob [n_pat]: metastasis / mass[1] at the row's MT genotype dat[:, 1:2*n:2], its probability among the metastases; NaN
        for the other types;
    founder_events [n_pat]: the expected number of the MT genotype's mutations the founder held; NaN for the other types;
    codes [n_pat]: the rows' MT genotype codes, -1 for the other types;
    table: {stratum: (codes, observed, expected)} for the strata with rows - the distinct genotype codes of the stratum's
        rows, ascending, how many rows carry each, and rows of the stratum x the genotype's probability;
    summary: the model.MetastasisSummary of the whole lattice;  residuals: summary.compare(dat)."""
    from types import SimpleNamespace
    from .model import MetMHN
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    n = (arr.shape[1] - 3) // 2
    typ = arr[:, -1]
    pick = np.isin(typ, (2, 3))
    got = MetMHN(log_theta, log_d_p, log_d_m).metastasis_distribution_at(arr[pick][:, 1:2 * n:2], backend)
    prob = np.full(arr.shape[0], np.nan)
    founder_events = np.full(arr.shape[0], np.nan)
    codes = np.full(arr.shape[0], -1, dtype=np.int64)
    codes[pick] = got.codes
    prob[pick] = got.metastasis / got.summary.mass[1]
    founder_events[pick] = got.founder_events
    table = _stratum_table((("EM-MT", 2), ("paired", 3)), typ, codes, prob)
    return SimpleNamespace(prob=prob, founder_events=founder_events, codes=codes, table=table, summary=got.summary,
                           residuals=got.summary.compare(arr))


def partner_forecast(log_theta, log_d_p, log_d_m, dat, backend: str = "device"):
    """What the model says of the tumour that was NOT sequenced, for every row of `dat` that holds one tumour of a
    metastasised (or possibly metastasised) patient, from MetMHN.partner_distributions with obs1 = log_d_p, obs2 = log_d_m
    (distinct genotypes are solved once).  A row of type 1 is taken as given PT (its PT genotype dat[:, 0:2*n:2]: what
    will the metastasis carry?), of type 2 as given MT (its MT genotype dat[:, 1:2*n:2]: what did the primary tumour look
    like?), of type 4 as given PT conditional on the seeding; rows of types 0 and 3 give NaN.  A namespace of
    frequencies [n_pat, n]: the conditional probability that the other tumour holds mutation j
        (PartnerSummary.conditional_frequencies);
    burden [n_pat]: its expected number of mutations;
    founder_burden [n_pat]: the founder's;
    mass [n_pat]: the probability of the row's own genotype (seeded, for the given PT);
    given [n_pat]: "PT", "MT" or "" per row;  codes [n_pat]: the genotype code the row was solved for, -1 for types 0 and 3;
    seeded [n_pat]: met_status_posterior's column - what a type-4 row's forecast is conditional on."""
    from types import SimpleNamespace
    from .model import MetMHN
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    n_pat, n = arr.shape[0], (arr.shape[1] - 3) // 2
    typ = arr[:, -1]
    mod = MetMHN(log_theta, log_d_p, log_d_m)
    if backend == "host":                                    # the same number without the library
        own = np.isin(typ, (0, 1, 4))
        seeded = np.full(n_pat, np.nan)
        seeded[own] = mod.genotype_distribution_at(arr[own][:, 0:2 * n:2], "host").p_seeded
    else:
        seeded = met_status_posterior(log_theta, log_d_p, log_d_m, dat)
    out = SimpleNamespace(frequencies=np.full((n_pat, n), np.nan), burden=np.full(n_pat, np.nan),
                          founder_burden=np.full(n_pat, np.nan), mass=np.full(n_pat, np.nan),
                          given=np.full(n_pat, "", dtype="<U2"), codes=np.full(n_pat, -1, dtype=np.int64), seeded=seeded)
    for given, pick, first in (("PT", np.isin(typ, (1, 4)), 0), ("MT", typ == 2, 1)):
        if not pick.any():
            continue
        got = mod.partner_distributions(arr[pick][:, first:2 * n:2], given, backend=backend)
        out.given[pick], out.codes[pick], out.mass[pick] = given, got.codes, got.mass
        out.frequencies[pick] = [s.conditional_frequencies("partner") for s in got.summaries]
        out.burden[pick] = [s.expected_burden("partner") for s in got.summaries]
        out.founder_burden[pick] = [s.expected_burden("founder") for s in got.summaries]
    return out


def paired_fit(log_theta, log_d_p, log_d_m, dat, backend: str = "device"):
    """How well the model's exact second moments of a seeded pair fit the paired rows (type 3) of `dat` - the counterpart
    of genotype_fit and metastasis_fit for what the two tumours of a patient share, from MetMHN.paired_summary with
    obs1 = log_d_p, obs2 = log_d_m.  A namespace of
    rows: the number of paired rows;
    residuals: summary.compare(dat), {"paired": [2n, 2n]} - the exact form of simulate_pairs(...).compare(dat)["paired"];
    shared, pt_private, mt_private: (observed [n], expected [n]) - how many paired rows hold mutation i in both tumours, in
        the primary tumour only, in the metastasis only, against rows x the model's probability (shared(), pt / mass -
        shared(), mt / mass - shared() of the CrossSummary);
    burden: {"pt", "mt", "shared": (observed mean, expected mean)} - the mean mutation counts of the paired rows against the
        marginals of burden_pmf() and expected_shared() (observed NaN without paired rows);
    summary: the results.PairedSummary."""
    from types import SimpleNamespace
    from .model import MetMHN
    arr = np.ascontiguousarray(np.asarray(dat).astype(np.int8))
    n = (arr.shape[1] - 3) // 2
    summary = MetMHN(log_theta, log_d_p, log_d_m).paired_summary(backend)
    cross = summary.cross
    rows = arr[arr[:, -1] == 3]
    pt, mt = rows[:, 0:2 * n:2].astype(np.int64), rows[:, 1:2 * n:2].astype(np.int64)
    R = rows.shape[0]
    both = cross.shared()
    only_pt, only_mt = cross.pt / cross.mass - both, cross.mt / cross.mass - both
    pmf, k = cross.burden_pmf(), np.arange(n + 1)
    mean = lambda v: float(v.mean()) if R else float("nan")
    burden = {"pt": (mean(pt.sum(axis=1)), float(k @ pmf.sum(axis=1))), "mt": (mean(mt.sum(axis=1)), float(k @ pmf.sum(axis=0))),
              "shared": (mean((pt & mt).sum(axis=1)), cross.expected_shared())}
    return SimpleNamespace(rows=R, residuals=summary.compare(arr), shared=((pt & mt).sum(axis=0), R * both),
                           pt_private=((pt & ~mt & 1).sum(axis=0), R * only_pt),
                           mt_private=((mt & ~pt & 1).sum(axis=0), R * only_mt), burden=burden, summary=summary)


def _unpack(params, n_total):
    params = np.asarray(params, dtype=np.float64)
    return (params[0:n_total ** 2].reshape((n_total, n_total)), params[n_total ** 2:n_total * (n_total + 1)],
            params[n_total * (n_total + 1):])


def score_reg(params, dat, perc_met: float, penal: Callable, w_penal: float, weights=None, groups=None):
    """regularized_optimization.py:133-160.  weights, groups: see score."""
    n_total = (np.asarray(dat).shape[1] - 3) // 2 + 1
    th, dp, dm = _unpack(params, n_total)
    eng = _weighted_engine(dat, weights, groups)
    res, (pen, _) = _result(eng, th, dp, dm, perc_met, False, meanwhile=lambda: penal(params, n_total), guard=dat)    # penalty next to the GPU
    return np.array(-res[0] + w_penal * pen)


def score_and_grad_reg(params, dat, perc_met: float, penal: Callable, w_penal: float, weights=None, groups=None):
    """regularized_optimization.py:270-298.  weights, groups: see score."""
    n_total = (np.asarray(dat).shape[1] - 3) // 2 + 1
    th, dp, dm = _unpack(params, n_total)
    eng = _weighted_engine(dat, weights, groups)
    (sc, d_th, d_d_p, d_d_m), (pen, pen_) = _result(eng, th, dp, dm, perc_met, True, meanwhile=lambda: penal(params, n_total), guard=dat)  # penalty next to the GPU
    grad_vec = np.concatenate((d_th.flatten(), d_d_p, d_d_m))
    return np.array(-sc + w_penal * pen), -grad_vec + w_penal * pen_


def learn_mhn(th_init, dp_init, dm_init, dat, perc_met: float, penal: Callable, w_penal: float,
              opt_iter: int = 1e05, opt_ftol: float = 1e-04, opt_v: bool = True, weights=None, groups=None):
    """Infer a metMHN with SciPy's L-BFGS-B (regularized_optimization.py:301-334).  weights, groups: see score."""
    th_init = np.asarray(th_init, dtype=np.float64)
    n_total = th_init.shape[0]
    start = np.concatenate((th_init.flatten(), np.asarray(dp_init, float), np.asarray(dm_init, float)))
    x = opt.minimize(fun=score_and_grad_reg, jac=True, x0=start, method="L-BFGS-B",
                     args=(dat, perc_met, penal, w_penal, weights, groups),
                     options={"maxiter": int(opt_iter), "disp": opt_v, "ftol": opt_ftol})
    theta = np.array(x.x[:n_total ** 2]).reshape((n_total, n_total))
    d_p = np.array(x.x[n_total ** 2:n_total * (n_total + 1)])
    d_m = np.array(x.x[n_total * (n_total + 1):])
    return theta, d_p, d_m


def impute_missing(log_theta, log_d_p, log_d_m, groups):
    """Posterior of the unobserved entries of a cohort (groups: a RowGroups from Utilityfunctions.expand_missing):
    (p [len(groups.entries)], lp [rows of the original dat]) with p[k] = P(entry k = 1 | the row's observed entries) - the
    sum of rho over the completions that set it - and lp the log-likelihood of every original row.  An entry in a column
    its row's type ignores was not expanded: NaN.  One score-only evaluation (Engine.group_posteriors)."""
    eng = _weighted_engine(groups.rows, None, groups)
    lpg, rho = eng.group_posteriors(log_theta, log_d_p, log_d_m)
    ptr = np.asarray(groups.ptr, dtype=np.int64)
    p = np.array([float(np.sum(rho[ptr[r] + np.asarray(alts, dtype=np.int64)])) if len(alts) else np.nan
                  for r, _, alts in groups.entries], dtype=np.float64)
    return p, lpg
