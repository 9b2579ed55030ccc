"""Several ranks and several devices: the in-library RCCL all-reduce, the sharded engine, explicit devices, and the BASELINE
multi-GPU configurations as one rank sees them.  References: the golden cohorts (the unsharded result of the reference),
oracle/metmhn_fast.c (cref.fast_patients) for rows of a shard, and the unsharded engine for partial sums."""
import numpy as np
import pytest

from eval_common import TIGHT, close, close_grads, fp32_close, free_port, one_rank_comm

pytestmark = pytest.mark.gpu


def test_in_library_rccl_allreduce_single_rank(monkeypatch, golden):
    """MMHN_FORCE_ALLREDUCE=1 with a 1-rank nccl group: Engine.cohort_sums -> k_pack_sums -> ncclAllReduce on the
    engine's stream (mmhn_comm_init) -> combine_sums, against the reference's cohort golden."""
    import torch
    import torch.distributed as dist
    import metmhn_amd.regularized_optimization as ro
    monkeypatch.setenv("MMHN_FORCE_ALLREDUCE", "1")
    monkeypatch.setenv("MMHN_STRICT_COMM", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        ro.configure(device=0)
        g = golden("cohorts")
        for c in (0, 1):
            pre = f"c{c}_"
            dat = g[pre + "dat"]
            res = ro.score_and_grad(g[pre + "log_theta"], g[pre + "log_d_p"], g[pre + "log_d_m"], dat, float(g[pre + "perc_met"]))
            eng = ro._engine_for(dat)
            assert eng._sharded and eng._device_comm
            close_grads(f"cohort {c}", res, [g[pre + s] for s in ("score", "d_th", "d_dp", "d_dm")], (1e-9, 0.0), TIGHT)
    finally:
        ro.configure()
        dist.destroy_process_group()


def _shard_worker(rank, world, port, q):
    """One rank of the sharded-engine test: real Engine on cuda:0 over its LPT shard; gloo carries the all-reduce
    (two ranks cannot share one GPU under RCCL)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import metmhn_amd.regularized_optimization as ro
    ro.configure(device=0)
    g = np.load(os.path.join(root, "tests", "golden", "cohorts.npz"))
    res = ro.score_and_grad(g["c1_log_theta"], g["c1_log_d_p"], g["c1_log_d_m"], g["c1_dat"], float(g["c1_perc_met"]))
    eng = ro._engine_for(g["c1_dat"])
    q.put((rank, eng.n_pat, [np.asarray(r) for r in res]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_engine_matches_golden(golden):
    """world_size 2, each rank a real engine over its own patient shard, one all-reduce: every rank gets the
    unsharded (reference) result."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    g = golden("cohorts")
    assert sorted(r[0] for r in got) == [0, 1]
    assert sum(r[1] for r in got) == g["c1_dat"].shape[0] and all(r[1] > 0 for r in got)
    for rank, _, res in got:
        close_grads(f"rank {rank}", res, [g["c1_" + s] for s in ("score", "d_th", "d_dp", "d_dm")], (1e-9, 0.0), TIGHT)


def test_engines_on_explicit_device_and_guard():
    """Every ABI entry selects the engine's GPU itself (DevGuard) and restores the caller's device."""
    import torch
    from metmhn_amd import Engine, synthetic
    n = 5
    lt, dp, dm = synthetic.random_params(n)
    dat = synthetic.mixed_cohort(n, 20, seed=9)
    with Engine(n, device=0) as e:
        e.set_cohort(dat)
        r0 = e.patient_grads(lt, dp, dm, with_grad=False)
        assert torch.cuda.current_device() == 0
        with Engine(n) as e2:                  # default device: LOCAL_RANK or 0
            e2.set_cohort(dat)
            close("default device against device 0", e2.patient_grads(lt, dp, dm, with_grad=False), r0, 1e-13)
    with pytest.raises(RuntimeError):
        Engine(n, device=10_000)


def test_config3_rank_shard_n20_50000_patients():
    """BASELINE configs[3] (n = 20, 50 000 patients over 8 GPUs) as ONE rank sees it: the LPT shard 0 of the 50 000-row
    cohort (6 250 rows, regularized_optimization.py:256-266 is what shards), evaluated through the pre-combined
    all-reduce payload with the in-library RCCL all-reduce attached; 8 random rows of the shard against
    oracle/metmhn_fast.c, and the shard's weighted sums against the sum of its per-patient rows."""
    from oracle import cref
    from metmhn_amd import Engine, synthetic, distributed as D
    n, P, W = 20, 50000, 8
    lt, dp, dm = synthetic.random_params(n)
    dat = synthetic.full_k_cohort(n, P, seed=2000 + n)
    parts = D.shard_rows(dat, W)
    assert sorted(np.concatenate(parts).tolist()) == list(range(P)) and max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    rows = dat[parts[0]]
    assert rows.shape[0] == P // W
    w, n_full = D.em_weight(float(dat[:, -3].sum()), float(P), 0.5)
    with Engine(n) as e:
        e.set_cohort(rows)
        one_rank_comm(e)
        e.cohort_wsums_begin(lt, dp, dm, w)
        ws = e.cohort_wsums_end()
        got = e.patient_grads(lt, dp, dm)
    lp, g, gp, gm = got
    N = n + 1
    assert ws.shape == (1 + N * N + 2 * N,) and np.isfinite(ws).all()
    # every row is a paired (EM) patient: the payload is w times the plain sums of the shard's rows
    close("payload score", ws[0], w * lp.sum(), 1e-11)
    close("payload d_theta", ws[1:1 + N * N].reshape(N, N), w * g.sum(axis=0), 1e-9, 1e-9)
    close("payload d_dp", ws[1 + N * N:1 + N * N + N], w * gp.sum(axis=0), 1e-9, 1e-9)
    close("payload d_dm", ws[1 + N * N + N:], w * gm.sum(axis=0), 1e-9, 1e-9)
    pick = np.random.default_rng(5).choice(rows.shape[0], size=8, replace=False)
    close_grads("8 rows of the shard", [x[pick] for x in got], cref.fast_patients(lt, dp, dm, rows[pick]), (1e-10, 0.0), (1e-7, 1e-10))


def test_shard_partial_sums_add_up():
    """8 LPT shards of a 64-row mixed cohort (all dat types), each evaluated by an engine of its own with the
    collective attached: the 8 partial buffers add up to the unsharded buffer to 1e-12 - both layouts (raw sums and
    the pre-combined payload)."""
    from metmhn_amd import Engine, synthetic, distributed as D
    n = 7
    lt, dp, dm = synthetic.random_params(n, seed=21)
    dat = np.vstack((synthetic.mixed_cohort(n, 48, seed=4, p_event=0.45), synthetic.full_k_cohort(n, 16, seed=9)))
    w, n_full = D.em_weight(float(dat[:, -3].sum()), float(dat.shape[0]), 0.3)
    with Engine(n) as e:
        e.set_cohort(dat)
        full = e.cohort_sums(lt, dp, dm)
        e.cohort_wsums_begin(lt, dp, dm, w)
        wfull = e.cohort_wsums_end()
    acc, wacc = np.zeros_like(full), np.zeros_like(wfull)
    for part in D.shard_rows(dat, 8):
        with Engine(n) as e:
            e.set_cohort(dat[part])
            one_rank_comm(e)
            acc += e.cohort_sums(lt, dp, dm)
            e.cohort_wsums_begin(lt, dp, dm, w)
            wacc += e.cohort_wsums_end()
    close("raw sums of the shards", acc, full, 1e-12, 1e-12)
    close("payloads of the shards", wacc, wfull, 1e-12, 1e-12)
    close_grads("split payload against combined sums", D.split_wsums(wacc, n + 1, n_full), D.combine_sums(full, n + 1, 0.3), (1e-11, 1e-13), (1e-11, 1e-13))


def test_config4_rank_shard_n25_fp32_multi_batch():
    """BASELINE configs[4] (n = 25, 10 000 patients, fp32, 8 GPUs) as ONE rank sees it: the 1 250-row LPT shard 0 -
    2 x 1 250 x 128 MiB of solution vectors do not fit the workspace, so the engine runs it in several batches - with
    the collective attached; 8 random rows against oracle/metmhn_fast.c (fp64) at the fp32 bar: log-prob 1e-4,
    every gradient component within 2e-3 relative + 2e-5 absolute; the payload equals the sum of the per-patient rows."""
    from oracle import cref
    from metmhn_amd import Engine, synthetic, distributed as D
    n, P, W = 25, 10000, 8
    lt, dp, dm = synthetic.random_params(n)
    dat = synthetic.full_k_cohort(n, P, seed=2000 + n)
    part = D.shard_rows(dat, W)[0]
    rows = dat[part]
    assert rows.shape[0] == P // W
    w, n_full = D.em_weight(float(dat[:, -3].sum()), float(P), 0.5)
    with Engine(n, dtype="f32") as e:
        e.set_cohort(rows)
        one_rank_comm(e)
        e.cohort_wsums_begin(lt, dp, dm, w)
        ws = e.cohort_wsums_end()
        lp, g, gp, gm = e.patient_grads(lt, dp, dm)
    N = n + 1
    assert np.isfinite(ws).all() and np.isfinite(lp).all()
    close("payload score", ws[0], w * lp.sum(), 1e-9)
    # (two fp32 evaluations, 1 250 terms per sum: agreement to fp32 rounding of the partial sums)
    close("payload d_theta", ws[1:1 + N * N].reshape(N, N), w * g.sum(axis=0), 2e-5, 2e-5)
    pick = np.random.default_rng(6).choice(rows.shape[0], size=8, replace=False)
    rlp, rg, ra, rb = cref.fast_patients(lt, dp, dm, rows[pick])
    close("lp", lp[pick], rlp, 1e-4)
    for tag, x32, x64 in (("d_theta", g[pick], rg), ("d_dp", gp[pick], ra), ("d_dm", gm[pick], rb)):
        fp32_close(tag, x32, x64)


def _rccl_worker(rank, world, port, q):
    """One rank of the in-library RCCL test: its own GPU, backend nccl, MMHN_STRICT_COMM=1 (no fallback to torch's
    collective), the golden cohort c0 sharded over the ranks."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["MMHN_STRICT_COMM"] = "1"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    import metmhn_amd.regularized_optimization as ro
    ro.configure(device=rank)
    g = np.load(os.path.join(root, "tests", "golden", "cohorts.npz"))
    res = ro.score_and_grad(g["c0_log_theta"], g["c0_log_d_p"], g["c0_log_d_m"], g["c0_dat"], float(g["c0_perc_met"]))
    eng = ro._engine_for(g["c0_dat"])
    q.put((rank, eng.n_pat, bool(eng._device_comm), [np.asarray(r) for r in res]))
    dist.barrier()
    dist.destroy_process_group()


def test_in_library_rccl_two_ranks(golden):
    """The first multi-rank run of the in-library all-reduce (ncclCommInitRank with two ranks, one ncclAllReduce of the
    pre-combined 1 + N^2 + 2N doubles per evaluation on each engine's stream): two processes, one GPU each, started before
    anything touches a GPU here.  Needs two GPUs: skipped on a one-GPU box, runs by itself on any multi-GPU box.
    Result of every rank == the unsharded reference result to 1e-12."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_rccl_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=600) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    g = golden("cohorts")
    assert sorted(r[0] for r in got) == [0, 1]
    assert all(r[2] for r in got), "the device communicator was not attached"
    assert sum(r[1] for r in got) == g["c0_dat"].shape[0]
    for rank, _, _, res in got:
        close_grads(f"rank {rank}", res, [g["c0_" + s] for s in ("score", "d_th", "d_dp", "d_dm")], (1e-12, 0.0), (1e-12, 1e-14))
