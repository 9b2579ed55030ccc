"""k_wsolve takes the move along external bit 0 from the thread's own window slot instead of global memory (csrc/wsolve.h:
own_take, and the invariant written at Wd).  An index-only model of begin_pass / step - no values, no GPU - walks the passes
of one lane as the kernel does and tags every window slot with the (patient, external index) of the block written into it;
whenever the bit-0 move exists on an active lane, the slot must hold the block of the same patient at Sigma ^ 1.  The scalar
schedule model the kernel comment cites (oracle/wschedule.py) is run unmodified on its own configurations."""
import pytest

WLB = 6                                      # lane bits of a thread (csrc/wlayout.h)
H = 4                                        # blocks of a window (fp64 and fp32)
NPAT = 3                                     # patients of the chain


def walk(m, nX, tr, npat=NPAT):
    """The passes of a lane of popcount m over a chain of `npat` patients with nX external bits; returns the number of bit-0
    moves it checked.  Mirrors begin_pass (V, act, j, g, Sigma) and step (beta, the slot written at the very end)."""
    if nX == 0:
        return 0                             # no external bit: the step takes no external term at all
    NXS = 1 << nX
    delay = WLB - m if tr else m             # lane-level: window passes the lane runs behind
    tag = [None] * H                         # (patient, Sigma) of the block a slot holds; None: zeros / an inactive pass
    moves = 0
    for sig in range(npat * NXS + WLB):      # NPASS
        V = sig - delay
        act = 0 <= V < npat * NXS
        Vc = V if act else 0
        j, g = Vc >> nX, Vc & (NXS - 1)
        Sigma = NXS - 1 - g if tr else g
        has0 = not (Sigma & 1) if tr else bool(Sigma & 1)
        if act and g == 0:
            # a lane's first pass of a patient: the slot holds the previous patient's last block (or nothing) and the move
            # must not exist - forward g = 0, transposed Sigma all ones
            assert not has0, (m, nX, tr, sig)
            assert Sigma == (NXS - 1 if tr else 0)
        for BI in range(H):
            beta = H - 1 - BI if tr else BI
            if act and has0:
                assert tag[beta] == (j, Sigma ^ 1), (m, nX, tr, sig, beta, tag[beta], (j, Sigma ^ 1))
                moves += 1
            tag[beta] = (j, Sigma) if act else None   # the step's last act: Wd[beta] = Y (an inactive lane leaves rubbish)
    return moves


@pytest.mark.parametrize("tr", [False, True], ids=["forward", "transposed"])
@pytest.mark.parametrize("nX", range(1, 10))
def test_bit0_source_is_in_the_own_slot(nX, tr):
    for m in range(WLB + 1):
        moves = walk(m, nX, tr)
        assert moves == NPAT * (1 << (nX - 1)) * H, (m, nX, tr, moves)     # half of the passes of every patient, every block


@pytest.mark.parametrize("tr", [False, True], ids=["forward", "transposed"])
def test_one_patient_and_no_external_bit(tr):
    for m in range(WLB + 1):
        assert walk(m, 0, tr) == 0                                          # nX = 0: no external move at all
        assert walk(m, 1, tr, npat=1) == H


@pytest.mark.parametrize("tr", [False, True], ids=["forward", "transposed"])
@pytest.mark.parametrize("cfg", [(2, 1, 1, 1, 1, 0), (2, 2, 1, 2, 1, 1), (3, 2, 2, 1, 2, 0), (3, 1, 1, 2, 0, 2), (2, 2, 2, 2, 2, 1)])
def test_schedule_model_unmodified(cfg, tr):
    from oracle import wschedule
    err, _ = wschedule.emulate(*cfg, tr)
    assert err < 1e-13, (cfg, tr, err)
