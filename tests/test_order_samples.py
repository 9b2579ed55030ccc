"""Posterior samples of event orders (MetMHN.sample_order / sample_orders, mmhn_order_samples, OrderSamples.preseeding /
.precedence, metmhn_amd/_philox.py).

Anchors:
  * the host draw against brute force over MetMHN.likelihood (pinned to the reference by tests/golden/orders.npz): every
    sampled order is admissible, carries exp(log_evidence + log_prob) = its likelihood, and comes as often as
    likelihood / Z says;
  * the device kernel against the host draw, sample by sample, on the samples whose host margin says that a last-bit
    difference of a weight (exp may round differently on the device) cannot change them;
  * on rows too slow for a live comparison with the host code (k >= 15), the device's samples against the host's of
    tests/golden/orders_big.npz on the synthetic rows, and on all of them the sample means against the exact marginals of
    order_posteriors and order_precedences, which the samples do not share a reduction with.
What sample_orders shares with the other cohort entry points: order_common.check_* and tests/test_order_contract.py.

Bars.  Statistical: a frequency of M samples against its exact probability p, |freq - p| <= 5 sqrt(p (1 - p) / M) + 1 / M.
Numerical: 1e-12 relative for what the host computes twice (likelihoods, totals), 1e-10 for log_prob between device and
host (a sum of at most k logs of quotients that differ by a few ulp) and for the device's likelihoods of large rows.  The
keys are fixed in tests/order_common.py.  Every test prints the worst value it saw before it asserts.
"""
import itertools
import warnings

import numpy as np
import pytest

from metmhn_amd import _philox
from metmhn_amd.model import OrderSamples
from metmhn_amd.state import MetState
from order_common import (BIG_SAMPLES, ENTRIES, FIRST, KEY, MARGIN, MAX_EXCLUDED, all_orders, big_models, check_arguments_before_the_library,
                          check_big_samples, check_errors_name_the_row, check_too_large_rows_get_the_host_value, large_rows, luad, luad_selection, model,
                          random_paired_states, row, small_shapes_n8)

ENTRY = ENTRIES["sample_orders"]


def _bound(p, M):
    """The statistical bar of this file: p the exact probability (a quotient of two roundings may pass 1), M samples."""
    p = np.clip(p, 0.0, 1.0)
    return 5.0 * np.sqrt(p * (1.0 - p) / M) + 1.0 / M


def _check_against_enumeration(mod, got, orders, status, first, M):
    """The three checks of a host draw against every admissible order: returns (worst relative difference of
    exp(log_evidence + log_prob) from the order's likelihood, worst (|freq - p| - bound), samples outside the orders)."""
    Z = np.exp(got.log_evidence)
    like = {tuple(o): mod.likelihood(o, status, first) for o in orders}
    assert abs(sum(like.values()) - Z) <= 1e-12 * Z
    uniq, inverse, counts = np.unique(got.orders, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.ravel()
    keys = [tuple(int(c) for c in u if c >= 0) for u in uniq]
    for u, key in zip(uniq, keys):                                            # padded with -1, nothing behind the padding
        assert np.all(u[len(key):] == -1)
    outside = sum(int(c) for key, c in zip(keys, counts) if key not in like)
    lk = np.array([like.get(key, np.nan) for key in keys])
    rel = np.abs(np.exp(got.log_evidence + got.log_prob) - lk[inverse]) / lk[inverse]
    seen = dict(zip(keys, counts))
    over = max(abs(seen.get(o, 0) / M - p / Z) - _bound(p / Z, M) for o, p in like.items())
    return float(rel.max(initial=0.0)), float(over), outside


# ---------------------------------------------------------------------------------------------------- CPU
def test_philox_known_answers_and_the_replay_generator():
    """Random123's published known answers for philox4x32-10 (those of tests/test_sampler_replay.py), and the generator of
    oracle/sampler_replay.py on 1 000 random counters."""
    from oracle import sampler_replay as R
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(int(v) for v in _philox.philox4x32_10(*ctr, *key)) == out
    rng = np.random.default_rng(7)
    words = rng.integers(0, 2 ** 32, (6, 1000), dtype=np.uint64)
    mine, theirs = _philox.philox4x32_10(*words), R.philox4x32_10(*words)
    for a, b in zip(mine, theirs):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(_philox.uniform53(mine[0], mine[1]), R.uniform53(theirs[0], theirs[1]))
    assert _philox.uniform53(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    # the stream of the order samples: key = the seed, counter = (sample low, sample high, move, row + 1)
    ids = np.array([0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3], dtype=np.uint64)
    r0, r1, _, _ = R.philox4x32_10(ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32), 4, 18, KEY & 0xFFFFFFFF, KEY >> 32)
    np.testing.assert_array_equal(_philox.order_uniforms(KEY, 17, ids, 4), R.uniform53(r0, r1))


def test_arguments_are_checked_before_the_library(monkeypatch):
    mod = check_arguments_before_the_library(ENTRY, monkeypatch)
    dat = np.array([row(5, [0, 4, 6], 0), row(5, [0, 1, 10], 3, 1)])
    for kw in (dict(n_samples=-1), dict(n_samples=4, first=-1)):
        with pytest.raises(ValueError, match="n_samples and first must be non-negative"):
            mod.sample_orders(dat, **kw)
        with pytest.raises(ValueError, match="n_samples and first must be non-negative"):
            mod.sample_order(MetState([0, 4, 6], size=11), "absent", **kw)


@pytest.mark.parametrize("n", [4, 5])
def test_one_tumour_rows_against_enumeration(n):
    """sample_order of "isMetastasis", "present" and "absent" states with k = 0 ... 5 slots, 20 000 samples each, against
    every permutation."""
    M, S = 20000, 2 * n
    mod = model(n, seed=500 + n)
    worst = {"likelihood": 0.0, "freq - bound": -np.inf, "total": 0.0}
    cases = 0
    for k in range(6):
        todo = []
        if k >= 1:
            ev = [2 * i for i in range(n)][n - k + 1:]                        # k - 1 mutations and the seeding
            todo += [(ev + [S], "isMetastasis"), (ev + [S], "present")]
        if k <= n:
            todo.append(([2 * i for i in range(k)], "absent"))
        for sl, status in todo:
            assert len(sl) == k
            state = [s + 1 if status == "isMetastasis" and s != S else s for s in sl]
            got = mod.sample_order(MetState(state, size=S + 1), status, n_samples=M, key=KEY + k, first=FIRST, row=cases)
            assert got.orders.shape == (M, S + 1) and got.orders.dtype == np.int8 and got.log_prob.shape == (M,)
            rel, over, outside = _check_against_enumeration(mod, got, list(itertools.permutations(sorted(state))), status, None, M)
            assert outside == 0, (sl, status)                                 # every order a permutation of the row's codes
            # the total of every move against B[x] = G[x] den[x] of the state the move leaves
            theta, after = (mod.log_theta, mod.obs2) if status == "isMetastasis" else (mod._pt_log_theta, mod.obs1)
            T = mod._single_tables(theta, MetState(state, size=S + 1).MT if status == "isMetastasis"
                                   else MetState(state, size=S + 1).PT_S, after)
            _, _, G = mod._single_passes(T)
            slot = {c: b for b, c in enumerate(sorted(state))}
            x = np.zeros(M, dtype=np.int64)
            for move in range(k):
                B = G[x] * T.den[x]
                worst["total"] = max(worst["total"], float((np.abs(got.totals[:, move] - B) / B).max()))
                x |= 1 << np.array([slot[int(c)] for c in got.orders[:, move]])
            worst["likelihood"], worst["freq - bound"] = max(worst["likelihood"], rel), max(worst["freq - bound"], over)
            cases += 1
    print(f"one-tumour rows against enumeration, n = {n}: {cases} cases of {M} samples, worst {worst}")
    assert cases == (15 if n == 4 else 16)
    assert worst["likelihood"] <= 1e-12
    assert worst["freq - bound"] <= 0.0
    assert worst["total"] <= 1e-12


def test_sample_means_of_known_orders():
    """preseeding / precedence on hand-made samples: a joint event before the seeding happens at one moment."""
    n = 3
    S = 2 * n
    pad = lambda o: list(o) + [-1] * (S + 1 - len(o))
    paired = [pad([0, 1, S, 2, 5]), pad([S, 0, 1, 2, 5]), pad([0, 1, S, 5, 2]), pad([S, 5, 2, 1, 0])]
    met = [pad([1, S, 3]), pad([S, 3, 1]), pad([3, 1, S]), pad([1, 3, S])]
    absent = [pad([0, 4])] * 4
    run = OrderSamples(np.zeros(3), np.array([paired, met, absent], dtype=np.int8), np.zeros((3, 4)))
    pre, prec = run.preseeding(), run.precedence()
    np.testing.assert_array_equal(pre[0], [0.5, 0.0, 0.0])
    np.testing.assert_array_equal(pre[1], [0.75, 0.5, 0.0])
    assert np.all(np.isnan(pre[2]))
    assert prec.shape == (3, S + 1, S + 1)
    assert prec[0, 0, 1] == 0.25 and prec[0, 1, 0] == 0.25                     # together twice, apart twice
    assert prec[0, 0, S] == 0.5 and prec[0, S, 0] == 0.5 and prec[0, 1, S] == 0.5
    assert prec[0, 2, 5] == 0.5 and prec[0, S, 5] == 1.0 and prec[0, 5, 5] == 0.0
    assert np.all(np.isnan(prec[0, 3])) and np.all(np.isnan(prec[0, :, 4]))
    assert prec[1, 1, 3] == 0.5 and prec[1, 3, S] == 0.5 and prec[1, 1, S] == 0.75
    assert prec[2, 0, 4] == 1.0 and prec[2, 4, 0] == 0.0 and np.isnan(prec[2, 0, S])
    empty = OrderSamples(np.zeros(2), np.zeros((2, 0, S + 1), dtype=np.int8), np.zeros((2, 0)))
    assert np.all(np.isnan(empty.preseeding())) and np.all(np.isnan(empty.precedence()))


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_host_against_enumeration_paired(n):
    """Random paired states with k <= 7, all four first_obs values, 20 000 samples each; events only in PT, only in MT and in
    both must all occur.  (The diagonal of a paired state comes from the device.)"""
    M, S = 20000, 2 * n
    worst = {"likelihood": 0.0, "freq - bound": -np.inf, "|total - 1|": 0.0}
    cases = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for drawn, (mod, slots, seen) in enumerate(random_paired_states(n, 140 + n, (600 + n,), 6), start=1):
            state = MetState(slots + [S], size=S + 1)
            orders = list(all_orders(state))
            for first in ("PT", "Met", "unknown", "sync"):
                got = mod.sample_order(state, "isPaired", first, n_samples=M, key=KEY ^ drawn, first=FIRST, row=cases)
                rel, over, outside = _check_against_enumeration(mod, got, orders, "isPaired", first, M)
                # (outside == 0: every event before the seeding came as the adjacent pair 2i, 2i+1 - all_orders has no
                # other orders)
                assert outside == 0, (slots, first)
                o = got.orders.astype(np.int64)
                sp = (o == S).argmax(axis=1)
                assert np.all(sp % 2 == 0)
                for j in range(0, int(sp.max()), 2):
                    pair = sp > j
                    assert np.all(o[pair, j] % 2 == 0) and np.all(o[pair, j + 1] == o[pair, j] + 1)
                moves = np.arange(got.totals.shape[1])
                after = (moves[None, :] > sp[:, None] // 2) & ~np.isnan(got.totals)
                worst["|total - 1|"] = max(worst["|total - 1|"], float(np.abs(got.totals[after] - 1.0).max(initial=0.0)))
                worst["likelihood"], worst["freq - bound"] = max(worst["likelihood"], rel), max(worst["freq - bound"], over)
                cases += 1
    print(f"paired host against enumeration, n = {n}: {cases} cases of {M} samples, events {seen}, worst {worst}")
    assert cases == 24 and min(seen.values()) > 0
    assert worst["likelihood"] <= 1e-12
    assert worst["freq - bound"] <= 0.0
    assert worst["|total - 1|"] <= 1e-12


@pytest.fixture(scope="module")
def small_run():
    """The small shapes: 300 samples per row from the device and from the host, row by row (with the margins)."""
    mod, dat = small_shapes_n8()
    dev = mod.sample_orders(dat, 300, key=KEY, first=FIRST)
    assert mod.samples_fallback_rows == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        host = [mod.sample_order(*mod._row_args(dat, i), n_samples=300, key=KEY, first=FIRST, row=i) for i in range(len(dat))]
    return mod, dat, dev, host


@pytest.mark.gpu
def test_device_against_host_small_shapes(small_run):
    """300 samples per row (the second pass of the 256-thread loop partly filled), sample indices from 2^32 - 100, a seed
    with a high word.  The host alone stays far inside the cap on the excluded samples: a uniform lands within 1e-9 of one
    of at most k boundaries with chance <= 2e-9 k per move, under 3e-7 per sample of k <= 11 moves."""
    mod, dat, dev, host = small_run
    k = dat[:, :-2].astype(int).sum(1)
    assert set(int(v) for v in k) >= {0, 1, 2, 3, 6, 7, 8, 9, 10, 11} and k.max() <= 11
    assert dev.orders.shape == (len(dat), 300, 2 * mod.n + 1) and dev.orders.dtype == np.int8
    assert dev.log_prob.shape == (len(dat), 300)
    le = np.array([h.log_evidence for h in host])
    rel = np.abs(np.exp(dev.log_evidence) - np.exp(le)) / np.exp(le)
    margin = np.array([h.margin for h in host])
    safe = margin >= MARGIN
    same = np.array([(h.orders == dev.orders[i]).all(axis=1) for i, h in enumerate(host)])
    d_lp = np.abs(np.array([h.log_prob for h in host]) - dev.log_prob)
    excluded = int((~safe).sum())
    print(f"device against host, small shapes: {len(dat)} rows x 300 samples, {excluded} set aside (smallest margin "
          f"{margin.min():.2e}), {int((~same & safe).sum())} of the others differ, worst |log_prob| difference "
          f"{d_lp[safe & same].max():.2e}, rel. evidence {rel.max():.2e}")
    assert excluded <= MAX_EXCLUDED * safe.size
    assert np.all(same[safe])
    assert d_lp[safe].max() <= 1e-10
    assert rel.max() <= 1e-12
    # every order holds the row's codes once, the seeding where the row has it, padded with -1
    for i, r in enumerate(dat):
        codes = np.flatnonzero(r[:2 * mod.n + 1])
        o = np.sort(dev.orders[i].astype(int), axis=1)
        assert np.all(o[:, len(o[0]) - len(codes):] == codes) and np.all(o[:, :len(o[0]) - len(codes)] == -1), i


@pytest.mark.gpu
def test_big_rows_against_host_values():
    """The synthetic rows of tests/golden/orders_big.npz, k = 15 ... 17 (the 1 024-thread instantiation), 64 samples each,
    with the comparison of test_device_against_host_small_shapes against the host's samples the fixture holds."""
    device = {}
    for name, m in big_models(synthetic_only=True):
        device[name] = m.mod.sample_orders(m.dat, BIG_SAMPLES, key=KEY + m.n, first=FIRST)
        assert m.mod.samples_fallback_rows == 0
    check_big_samples(device, MARGIN, MAX_EXCLUDED)


def _check_means(tag, mod, dat, run, M):
    """preseeding() and precedence() of the samples against the exact marginals of the same rows."""
    post, prec = mod.order_posteriors(dat), mod.order_precedences(dat).prec
    assert mod.posteriors_fallback_rows == 0 and mod.precedences_fallback_rows == 0
    worst = {}
    for name, est, exact in (("pre", run.preseeding(), post.pre), ("prec", run.precedence(), prec)):
        np.testing.assert_array_equal(np.isnan(est), np.isnan(exact), err_msg=f"{tag}: {name}")
        have = ~np.isnan(exact)
        worst[name] = float((np.abs(est[have] - exact[have]) - _bound(exact[have], M)).max())
        worst[name + " entries"] = int(have.sum())
    worst["log_evidence"] = float(np.abs(run.log_evidence - post.log_evidence).max())
    print(f"sample means against the exact marginals, {tag}: {len(dat)} rows x {M} samples, worst (|mean - p| - bound) and "
          f"entries {worst}")
    assert worst["pre"] <= 0.0 and worst["prec"] <= 0.0
    assert worst["log_evidence"] <= 1e-12


def _check_likelihoods(tag, mod, dat, run, count):
    """exp(log_evidence + log_prob) of the first `count` samples of every row against MetMHN.likelihood of their orders."""
    worst = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for i in range(len(dat)):
            _, status, first = mod._row_args(dat, i)
            done = {}
            for s in range(count):
                o = tuple(int(c) for c in run.orders[i, s] if c >= 0)
                if o not in done:
                    done[o] = mod.likelihood(o, status, first)
                worst = max(worst, abs(np.exp(run.log_evidence[i] + run.log_prob[i, s]) - done[o]) / done[o])
    print(f"likelihoods of sampled orders, {tag}: {len(dat)} rows x {count} samples, worst relative difference {worst:.2e}")
    assert worst <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("n, seed", [(9, 31), (16, 32)])
def test_large_synthetic_rows(n, seed):
    """4 096 samples per row against the exact marginals; the first 16 of them against the likelihoods of their orders."""
    dat = large_rows(n)
    k = dat[:, :-2].astype(int).sum(1)
    assert {14, 15, 16, 17} <= set(int(v) for v in k)
    mod = model(n, seed=seed)
    run = mod.sample_orders(dat, 4096, key=KEY + n, first=FIRST)
    assert mod.samples_fallback_rows == 0
    _check_likelihoods(f"synthetic n = {n}", mod, dat, run, 16)
    _check_means(f"synthetic n = {n}", mod, dat, run, 4096)


@pytest.mark.gpu
def test_luad_rows_against_the_exact_marginals(golden):
    """LUAD-28 at the fit point: the 71 rows with k >= 15 (k = 21 among them), 300 rows with k <= 12 and up to 200 with
    k = 13, 14; 256 samples per row."""
    mod, dat = luad(golden, "fit")
    sub = dat[luad_selection(dat)]
    k = sub[:, :-2].astype(int).sum(1)
    assert (k >= 15).sum() == 71 and k.max() == 21
    run = mod.sample_orders(sub, 256, key=KEY, first=FIRST)
    assert mod.samples_fallback_rows == 0
    _check_means("LUAD-28 fit", mod, sub, run, 256)


@pytest.mark.gpu
def test_reproducible_whatever_the_call(small_run):
    from metmhn_amd.engine import Engine
    from metmhn_amd.jx import engine
    mod, dat, dev, host = small_run
    args = (mod.log_theta, mod.obs1, mod.obs2)
    again = engine(mod.n).order_samples(*args, dat, 300, KEY, FIRST)
    assert np.all(again[3] == 0)
    for x, y in zip((dev.log_evidence, dev.orders, dev.log_prob), again):
        np.testing.assert_array_equal(x, y)
    # a sample depends on its index, not on the call that draws it
    part = engine(mod.n).order_samples(*args, dat, 70, KEY, FIRST + 50)
    np.testing.assert_array_equal(part[1], dev.orders[:, 50:120])
    np.testing.assert_array_equal(part[2], dev.log_prob[:, 50:120])
    # ... nor on the batch: a k = 11 paired row takes 152 KiB + 7 KiB of samples, the 65 rows many batches of 1 MiB
    with Engine(mod.n, workspace_bytes=1 << 20) as small:
        cut = small.order_samples(*args, dat, 300, KEY, FIRST)
    assert np.all(cut[3] == 0)
    for x, y in zip(again, cut):
        np.testing.assert_array_equal(x, y)
    # sample_order(row=i) is cohort row i
    safe = np.array([h.margin for h in host]) >= MARGIN
    for i, h in enumerate(host):
        np.testing.assert_array_equal(h.orders[safe[i]], dev.orders[i][safe[i]])
    # two identical rows at different indices draw different samples, a row at the same index the same
    twice = dat.copy()
    twice[11] = dat[10]
    le, orders, lp, _ = engine(mod.n).order_samples(*args, twice, 300, KEY, FIRST)
    assert le[10] == le[11] and (orders[10] != orders[11]).any() and (lp[10] != lp[11]).any()
    others = np.arange(len(dat)) != 11
    np.testing.assert_array_equal(orders[others], dev.orders[others])
    other = engine(mod.n).order_samples(*args, dat, 300, KEY + 1, FIRST)
    assert (other[1] != dev.orders).any()
    print(f"reproducible: {len(dat)} rows x 300 samples twice, a window of 70, batches of 1 MiB, {int(safe.sum())} samples "
          "against sample_order, a doubled row, another key")


@pytest.mark.gpu
def test_too_large_rows_get_the_host_samples(monkeypatch):
    """... with sample_order: the k = 14 row (1.2 MiB, over the 1 MiB workspace), what the device leaves in its place, and
    the host's samples against the device's own where the host margin allows."""
    mod, dat, ref, st, host = check_too_large_rows_get_the_host_value(ENTRY, monkeypatch)
    assert np.isnan(st[0][0]) and np.all(st[1][0] == -1) and np.all(np.isnan(st[2][0]))
    safe = host.margin >= MARGIN
    d_lp = np.abs(host.log_prob - ref.log_prob[0])[safe].max()
    print(f"host fallback, k = 14: {int(safe.sum())} of 64 samples compared with the device's, worst |log_prob| difference "
          f"{d_lp:.2e}")
    np.testing.assert_array_equal(host.orders[safe], ref.orders[0][safe])
    assert d_lp <= 1e-10


@pytest.mark.gpu
def test_errors_name_the_row_and_no_samples_is_valid():
    mod, good = check_errors_name_the_row(ENTRY)
    S = 2 * mod.n
    none = mod.sample_orders(good, 0)
    post = mod.order_posteriors(good)
    assert none.orders.shape == (len(good), 0, S + 1) and none.log_prob.shape == (len(good), 0)
    rel = np.abs(np.exp(none.log_evidence) - np.exp(post.log_evidence)) / np.exp(post.log_evidence)
    print(f"no samples: rel. difference of the evidences from order_posteriors' {rel.max():.2e}")
    assert rel.max() <= 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        host = mod.sample_orders(good, 5, key=3, backend="host")
    assert mod.samples_fallback_rows == 0 and host.orders.dtype == np.int8 and host.orders.shape == (len(good), 5, S + 1)
    np.testing.assert_allclose(host.log_evidence, post.log_evidence, rtol=0, atol=1e-12)
