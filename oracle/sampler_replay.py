"""Exact NumPy replay of the device Gillespie sampler - TEST INFRASTRUCTURE ONLY.

Restates what metmhn_amd/csrc/sampler.h documents (Philox4x32-10, counter = (trajectory low word, trajectory
high word, step, 0), key = (seed low word, seed high word); one uniform per step; `gillespie_step`) and the ABI
comments of include/metmhn_amd.h, with the process semantics of oracle/gillespie.py, so that every trajectory the
device draws can be compared event for event.  The floating-point operations are the kernel's, in its order:
  log-rate   diagonal entry, then + log_theta[e, j] for the set bits j ascending (bit * value for every j: adding
             0 is exact); the diagnosis row starts from 0
  rate       one exp
  total      rates summed one after the other, tumour 0 events 0..N then tumour 1 events 0..N
  u          (((r0 >> 5) << 26) | (r1 >> 6)) * 2^-53 * total
  event      first index with cum > u (the last positive rate if rounding leaves none)
Only `exp` may round differently on the device; `margin` says how far each trajectory's draws stayed from every
boundary, so a caller can set aside the (rare) trajectories a last-bit difference could decide.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

Replay = namedtuple("Replay", "dat orders counts margin trace")


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds.  Counter and key words as uint64 arrays (or ints) holding 32-bit values;
    returns the four output words as uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3, k0, k1))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 -> 64 bits, no overflow
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def uniform53(r0, r1):
    """The kernel's uniform in [0, 1): 27 high bits of r0 and 26 high bits of r1 as a 53-bit fraction."""
    m = ((r0 >> np.uint64(5)) << np.uint64(26)) | (r1 >> np.uint64(6))
    return m.astype(np.float64) * (1.0 / 9007199254740992.0)


def _log_rates(bits, rows, start):
    """start + sum over j ascending of bits[:, j] * rows[:, j]: [T, R] from bits [T, N], rows [R, N], start [R]."""
    s = np.broadcast_to(start, (bits.shape[0], rows.shape[0])).copy()
    for j in range(bits.shape[1]):
        s += bits[:, j, None] * rows[None, :, j]
    return s


def replay(log_theta, pt_d_ef, mt_d_ef, ids, seed, trace=False) -> Replay:
    """The trajectories `ids` (sample indices, any uint64 values) under the 64-bit key `seed`.

    dat     int8 [T, 2 n_mut + 2]   simulate_dat's rows
    orders  int8 [T, 2 N + 2]       simulate_orders' rows, padded with -99
    counts  int64 [4 + 5 n_mut]     mmhn_simulate_summary's vector over these trajectories
    margin  float64 [T]             min over the steps and the positive-rate boundaries j of |cum_j - u| / total
    trace   None, or per step a dict(alive, rates, u, event) for printing a divergence
    """
    lt = np.asarray(log_theta, dtype=np.float64)
    dp = np.asarray(pt_d_ef, dtype=np.float64)
    dm = np.asarray(mt_d_ef, dtype=np.float64)
    N = lt.shape[0]
    assert lt.shape == (N, N) and dp.shape == (N,) and dm.shape == (N,) and 2 <= N <= 31
    n_mut, L = N - 1, 2 * N + 2
    ids = np.asarray(ids).astype(np.uint64).ravel()
    T = ids.size
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    ltp = lt.copy()
    ltp[:-1, -1] = 0.0                                   # the seeding does not act on the PT's mutations
    diag = np.diag(lt).copy()
    zero = np.zeros(1)

    pt = np.zeros((T, N + 1), dtype=bool)                # events 0..N-1 (N-1 = seeding), N = diagnosed
    mt = np.zeros((T, N + 1), dtype=bool)
    pre = np.zeros((T, N + 1), dtype=bool)
    t_pt = np.full(T, -1)
    t_mt = np.full(T, -1)
    orders = np.full((T, L), -99, dtype=np.int8)
    margin = np.full(T, np.inf)
    alive = np.ones(T, dtype=bool)
    steps = [] if trace else None
    for step in range(L):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        p, m = pt[idx], mt[idx]
        pb, mb = p[:, :N].astype(np.float64), m[:, :N].astype(np.float64)
        r = np.empty((idx.size, L))
        r[:, :N] = np.exp(_log_rates(pb, ltp, diag))
        r[:, N:N + 1] = np.exp(_log_rates(pb, dp[None, :], zero))
        r[:, N + 1:L - 1] = np.exp(_log_rates(mb, lt, diag))
        r[:, L - 1:] = np.exp(_log_rates(mb, dm[None, :], zero))
        r[:, :N + 1][p] = 0.0                            # events that already happened
        r[:, N + 1:][m] = 0.0
        r[p[:, N], :N + 1] = 0.0                         # the PT is frozen once diagnosed
        r[~p[:, N - 1] | m[:, N], N + 1:] = 0.0          # the MT moves on its own only after the seeding
        cum = np.add.accumulate(r, axis=1)               # strictly sequential, as the kernel's loop
        total = cum[:, -1]
        r0, r1, _, _ = philox4x32_10(ids[idx] & _M32, ids[idx] >> _S32, np.uint64(step), np.uint64(0), k0, k1)
        u = uniform53(r0, r1) * total
        above = cum > u[:, None]
        last_pos = L - 1 - np.argmax(r[:, ::-1] > 0.0, axis=1)
        ev = np.where(above.any(axis=1), np.argmax(above, axis=1), last_pos)
        dist = np.where(r > 0.0, np.abs(cum - u[:, None]), np.inf).min(axis=1) / total
        margin[idx] = np.minimum(margin[idx], dist)
        if trace:
            steps.append(dict(alive=idx, rates=r, u=u, event=ev))

        orders[idx, step] = ev
        seeded = p[:, N - 1]
        in_pt = ev <= N
        a, e = idx[in_pt], ev[in_pt]
        seeding_now = e == N - 1
        pre[a[seeding_now]] = pt[a[seeding_now]]         # the PT set at the step that adds the seeding
        pt[a, e] = True
        both = ~seeded[in_pt]                            # before the seeding both tumours move together
        mt[a[both], e[both]] = True
        t_pt[a[e == N]] = step
        t_mt[a[both & (e == N)]] = step
        a, e = idx[~in_pt], ev[~in_pt] - (N + 1)
        mt[a, e] = True
        t_mt[a[e == N]] = step
        alive[idx] = ~(pt[idx, N] & (mt[idx, N] | ~pt[idx, N - 1]))
    assert not alive.any(), "a trajectory did not end within 2N + 2 steps"

    seeded = pt[:, N - 1]
    dat = np.zeros((T, 2 * n_mut + 2), dtype=np.int8)
    dat[:, 0:2 * n_mut:2] = pt[:, :n_mut]
    dat[:, 1:2 * n_mut:2] = mt[:, :n_mut]
    dat[:, 2 * n_mut] = seeded
    dat[:, 2 * n_mut + 1] = np.where(seeded, np.where(t_pt < t_mt, 1, 2), 0)
    P, M, S = pt[:, :n_mut], mt[:, :n_mut], seeded[:, None]
    head = [T, seeded.sum(), (dat[:, -1] == 1).sum(), (dat[:, -1] == 2).sum()]
    rows = [(pre[:, :n_mut] & S).sum(axis=0), (P & S).sum(axis=0), (M & S).sum(axis=0), (P & M & S).sum(axis=0),
            (P & ~S).sum(axis=0)]
    counts = np.concatenate([np.array(head, dtype=np.int64)] + [x.astype(np.int64) for x in rows])
    return Replay(dat, orders, counts, margin, steps)


def describe_step(rep: Replay, row: int, step: int) -> str:
    """The rates, u and event of trajectory `row` (position in `ids`) at `step` of a replay made with trace=True."""
    s = rep.trace[step]
    k = int(np.nonzero(s["alive"] == row)[0][0])
    with np.printoptions(precision=17, linewidth=200):
        return (f"step {step}: u = {s['u'][k]!r}, total = {s['rates'][k].sum()!r}, event {int(s['event'][k])}\n"
                f"rates = {s['rates'][k]}")
