"""The fp32 engine (dtype="f32", BASELINE configs[4]).  References: fp64 values - the CPU oracle and its C ports
(oracle/metmhn_oracle.py, metmhn_ref.c, metmhn_fast.c) or the fp64 engine on the same rows.  Bars: necessarily looser than the
1e-6 of fp64: log-probabilities 1e-4 relative, every gradient component at FP32_BAR, cohort scores 2e-5."""
import numpy as np
import pytest

from eval_common import FP32_BAR, close, close_grads, fp32_grads, patient_grads

pytestmark = pytest.mark.gpu


def test_fp32_engine_close_to_fp64():
    """dtype="f32" engine (BASELINE config 5 dtype) on a small cohort: looser tolerance by construction."""
    from oracle import metmhn_oracle as O
    from metmhn_amd import Engine, synthetic, distributed as D
    n = 6
    lt, dp, dm = synthetic.random_params(n)
    dat = np.vstack((synthetic.full_k_cohort(n, 6), synthetic.mixed_cohort(n, 40, seed=4)))
    with Engine(n, dtype="f32") as e:
        e.set_cohort(dat)
        res = D.combine_sums(e.cohort_sums(lt, dp, dm), n + 1, 0.5)
    close_grads("fp32 cohort against the oracle", res, O.score_and_grad(lt, dp, dm, dat, 0.5), (2e-5, 0.0), FP32_BAR)


def test_fp32_engine_tracks_fp64_engine_on_large_spaces(monkeypatch):
    """No CPU oracle finishes k = 18 in seconds: compare the fp32 engine (e_0 pre-scaled by 2^60) with the
    fp64 engine on the same paired patients; log-probs to 1e-4, every gradient component within 2e-3 relative +
    2e-5 absolute."""
    from metmhn_amd import synthetic
    n = 18
    params = synthetic.random_params(n)
    dat = synthetic.full_k_cohort(n, 6)
    r64, r32 = (patient_grads(monkeypatch, n, dat, params, dtype=dt) for dt in ("f64", "f32"))
    fp32_grads("k = 18", r32, r64)


def test_config4_n25_fp32_against_fp64_cpu(monkeypatch):
    """BASELINE configs[4] dtype and size: n = k = 25 (2^25-state vectors, 128 MiB fp32 each), engine dtype f32, against
    oracle/metmhn_fast.c in fp64.  fp32 bar (necessarily looser than 1e-6): log-prob 1e-4 relative, EVERY
    gradient component within 2e-3 relative + 2e-5 absolute (the worst component is printed).  Also one k = 22 patient:
    fp32 engine against the fp64 engine at the same bar."""
    from oracle import cref
    from metmhn_amd import synthetic
    n = 25
    params = synthetic.random_params(n)
    dat = synthetic.full_k_cohort(n, 3, seed=2025)
    fp32_grads("n=25", patient_grads(monkeypatch, n, dat, params, dtype="f32"), cref.fast_patients(*params, dat))
    n = 22
    params = synthetic.random_params(n)
    dat = synthetic.full_k_cohort(n, 1, seed=2022)
    r64, r32 = (patient_grads(monkeypatch, n, dat, params, dtype=dt) for dt in ("f64", "f32"))
    fp32_grads("k=22", r32, r64)


def test_batched_kronvec_and_jacobi_step_fp32():
    """The fp32 instantiations of the batched product and of the fused Jacobi step (BASELINE configs[4] runs the engine in
    fp32) against the fp64 CPU port at k = 16: 2e-5 of the vector's largest entry."""
    from oracle import cref, metmhn_oracle as O
    from metmhn_amd import Engine, synthetic
    cref.load()
    n = kk = 16
    lt, dp, dm = synthetic.random_params(n, seed=41)
    st = synthetic.full_k_cohort(n, 1, k=kk, seed=541)[0, :2 * n + 1]
    rng = np.random.default_rng(79)
    p = rng.random((3, 2 ** kk)) + 0.01
    rhs = rng.random((3, 2 ** kk))
    ones = np.ones(2 ** kk)
    lidg = 1.0 / (O.diag_scal_p(dp, st, ones) + O.diag_scal_m(dm, st, ones) - O.kron_diag(lt, st, kk))
    with Engine(n, dtype="f32") as e:
        for tr in (False, True):
            y = e.kronvec_batched(lt, p, st, diag=False, transpose=tr)
            z = e.jacobi_step_batched(lt, dp, dm, p, rhs, st, transpose=tr)
            for b in range(3):
                ref = cref.kronvec(lt, p[b], st, diag=False, transpose=tr)
                close(f"kronvec_batched transpose={tr} b={b}", y[b], ref, 0, 2e-5 * np.abs(ref).max())
                refz = lidg * (ref + rhs[b])
                close(f"jacobi_step_batched transpose={tr} b={b}", z[b], refz, 0, 2e-5 * np.abs(refz).max())


def test_small_space_path_fp32_on_luad_cohort(monkeypatch, golden):
    """The small-space kernels (csrc/small.h: side-by-side marginal problems, in-kernel marginal right-hand sides) in
    fp32 on the LUAD-reduced cohort, per patient against the fp64 C port (oracle/metmhn_ref.c, cref.patients - itself
    pinned to the reference on this cohort) at the fp32 bar: log-prob 1e-4 relative, every gradient component within
    2e-3 relative + 2e-5 absolute; the fp64 engine on the same rows against the same port at 1e-9."""
    from oracle import cref
    g = golden("luad_indep")
    dat, params = g["dat"], (g["indep_theta"], g["indep_dp"], g["indep_dm"])
    rows = np.concatenate((np.flatnonzero(dat[:, -1] == 3), np.arange(0, dat.shape[0], 23)))   # every paired row + a stride of the others
    sub = dat[rows]
    ref = cref.patients(*params, sub)
    n = (dat.shape[1] - 3) // 2
    close_grads("LUAD fp64", patient_grads(monkeypatch, n, sub, params), ref, (1e-9, 1e-12), (1e-9, 1e-12))
    fp32_grads("LUAD", patient_grads(monkeypatch, n, sub, params, dtype="f32"), ref, lp_atol=1e-5)
