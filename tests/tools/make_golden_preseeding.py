#!/usr/bin/env python3
"""Golden vectors for the reductions of simulated trajectories: the reference's `simulations.extract_bse` /
`preseeding_probs` (metmhn/simulations.py:150-240) and `Utilityfunctions.marg_frequs` (:116-155).

Runs ONLY in the build container, with the reference checkout on the path, under the NumPy jax stand-in:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=tests/tools/jax_standin:<reference checkout> \
    python tests/tools/make_golden_preseeding.py

jax drops out-of-bounds scatters, and the reference relies on that: `_extract_bse` clears `bsc.at[t]` for every
post-seeding event, also for t >= n.  The stand-in raises an IndexError there instead, so this tool (and only this
tool) wraps the stand-in's `.at[idx].set` to drop out-of-bounds indices.

The trajectories are built here, seeded: valid event sequences in simulate_orders' numbering (PT event e, MT event
e + N + 1, seeding N - 1, diagnoses N and 2N + 1, padded with -99 to 2N + 2), at N = 4 and N = 8.  They cover
unseeded trajectories, the seeding as the first and as the last mutation, PT and MT diagnosed first, and (N = 8)
one mutation that never occurs.  Writes tests/golden/preseeding.npz (data only: inputs + the reference's outputs):
  t{N}_traj [T, 2N+2] int8, t{N}_bsc [T, N], t{N}_tc [T, 2N+2]   extract_bse of every trajectory
  t{N}_pt [N-1], t{N}_mt [N-1]                                   preseeding_probs(traj, N, N-1)
  t{N}_unseeded_pt / _mt                                          preseeding_probs of the unseeded rows only (all NaN)
  mf_dat [P, 2n+3] int8, mf_events [n+1], mf_values [n+1, 6], mf_cols [6, 2]   marg_frequs(mf_dat, mf_events)
"""
import os
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "golden", "preseeding.npz")

import jax.numpy as jnp  # noqa: E402  (the stand-in)
from jax.numpy import _AtIdx  # noqa: E402

_set = _AtIdx.set


def _set_dropping(self, v):
    """`.at[idx].set(v)` with jax's default scatter mode: indices outside the array are dropped."""
    idx = self._idx
    size = np.asarray(self._arr).shape[0]
    if not isinstance(idx, (slice, tuple)):
        a = np.asarray(idx)
        if a.dtype.kind in "iu":
            keep = (a >= -size) & (a < size)
            if a.ndim == 0:
                if not keep:
                    return jnp.array(np.array(self._arr, copy=True))
            elif not keep.all():
                vv = np.asarray(v)
                return _set(_AtIdx(self._arr, a[keep]), vv[keep] if vv.ndim else vv)
    return _set(self, v)


_AtIdx.set = _set_dropping

import metmhn.simulations as rs  # noqa: E402
import metmhn.Utilityfunctions as ru  # noqa: E402


def trajectory(rng, N, never=()):
    """One valid event sequence of the joint process (simulate_orders' numbering), padded with -99."""
    muts = [m for m in range(N - 1) if m not in never]
    L = 2 * N + 2
    out = []
    kind = rng.random()
    order = list(rng.permutation(muts))
    if kind < 0.2:                                            # unseeded: PT diagnosed before the seeding
        out = order[:rng.integers(0, len(order) + 1)] + [N]
    else:
        if kind < 0.3:
            k = 0                                             # seeding is the first event
        elif kind < 0.4:
            k = len(order)                                    # seeding after every mutation
        else:
            k = int(rng.integers(0, len(order) + 1))
        pre, rest = order[:k], order[k:]
        out = pre + [N - 1]
        pt_rest = [m for m in rest if rng.random() < 0.5]
        mt_rest = [m for m in rest if rng.random() < 0.5]
        pt_seq = [int(m) for m in pt_rest] + [N]
        mt_seq = [int(m) + N + 1 for m in mt_rest] + [2 * N + 1]
        while pt_seq or mt_seq:                               # interleave; each tumour ends with its diagnosis
            take_pt = mt_seq == [] or (pt_seq != [] and rng.random() < 0.5)
            out.append((pt_seq if take_pt else mt_seq).pop(0))
    out = [int(e) for e in out]
    assert len(out) < L and len(set(out)) == len(out)
    return np.array(out + [-99] * (L - len(out)), dtype=np.int8)


def trajectories():
    out = {}
    for N, T, never in ((4, 1500, ()), (8, 2000, (5,))):
        rng = np.random.default_rng(20241016 + N)
        traj = np.stack([trajectory(rng, N, never) for _ in range(T)])
        seeded = (traj == N - 1).any(axis=1)
        diag_pt = np.argmax(traj == N, axis=1)
        diag_mt = np.where((traj == 2 * N + 1).any(axis=1), np.argmax(traj == 2 * N + 1, axis=1), -1)
        assert (~seeded).any() and (seeded & (diag_pt < diag_mt)).any() and (seeded & (diag_mt < diag_pt)).any()
        assert (traj[:, 0] == N - 1).any()
        bsc, tc = [], []
        for row in traj:
            b, t = rs.extract_bse(jnp.array(row), N, N - 1)
            bsc.append(np.asarray(b, dtype=np.int8))
            tc.append(np.asarray(t, dtype=np.int8))
        pt, mt = rs.preseeding_probs(jnp.array(traj), N, N - 1)
        upt, umt = rs.preseeding_probs(jnp.array(traj[~seeded]), N, N - 1)
        out.update({f"t{N}_traj": traj, f"t{N}_bsc": np.stack(bsc), f"t{N}_tc": np.stack(tc),
                    f"t{N}_pt": np.asarray(pt, dtype=np.float64), f"t{N}_mt": np.asarray(mt, dtype=np.float64),
                    f"t{N}_unseeded_pt": np.asarray(upt, dtype=np.float64),
                    f"t{N}_unseeded_mt": np.asarray(umt, dtype=np.float64)})
        print(f"N={N}: {T} trajectories, {int(seeded.sum())} seeded; pt {np.round(np.asarray(pt), 3)}")
    return out


def marg_frequs_case():
    rng = np.random.default_rng(7)
    n, P = 5, 300
    types = np.concatenate((np.arange(4), rng.integers(0, 4, size=P - 4)))
    dat = np.zeros((P, 2 * n + 3), dtype=np.int8)
    freq = rng.uniform(0.05, 0.6, size=n)
    for r, t in enumerate(types):
        pt = (rng.random(n) < freq).astype(np.int8)
        mt = np.where(rng.random(n) < 0.7, pt, (rng.random(n) < freq)).astype(np.int8)
        if t == 0:                                           # NM: PT only, no seeding
            dat[r, 0:2 * n:2] = pt
        elif t == 1:                                         # EM-PT: PT sequenced, seeding
            dat[r, 0:2 * n:2] = pt
            dat[r, 2 * n] = 1
        elif t == 2:                                         # EM-MT: MT sequenced, seeding
            dat[r, 1:2 * n:2] = mt
            dat[r, 2 * n] = 1
        else:                                                # coupled
            dat[r, 0:2 * n:2], dat[r, 1:2 * n:2], dat[r, 2 * n] = pt, mt, 1
            dat[r, 2 * n + 1] = rng.integers(0, 3)
        dat[r, -1] = t
    events = [f"E{i}" for i in range(n)] + ["Seeding"]
    df = ru.marg_frequs(dat, events)
    return {"mf_dat": dat, "mf_events": np.array(events), "mf_values": df.to_numpy(dtype=np.float64),
            "mf_cols": np.array([list(c) for c in df.columns])}


if __name__ == "__main__":
    out = trajectories()
    out.update(marg_frequs_case())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
