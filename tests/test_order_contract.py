"""The contract every cohort entry point of the order family keeps (MetMHN.order_posteriors, order_precedences,
order_positions, sample_orders), one test for all of them over order_common.ENTRIES: the C symbol, and bitwise equal results
whatever the batching.  The rest of the contract - the argument checks ahead of the library, the row errors of
likeliest_orders, the host value of a row the device turns away - is order_common.check_*, called by a test in every entry
point's own file, which goes on with what only that entry point has.  The bars are those of tests/test_order_posteriors.py.
"""
import os
import re

import numpy as np
import pytest

from metmhn_amd import _lib
from order_common import ENTRIES, luad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("e", ENTRIES.values(), ids=ENTRIES)
def test_abi_carries_the_symbol_and_version_8(e):
    hdr = open(os.path.join(ROOT, "include", "metmhn_amd.h")).read()
    assert e.symbol in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[e.symbol]) == e.n_args
    assert re.search(r"\bint %s\s*\(" % e.symbol, hdr)
    assert _lib.ABI_VERSION == 8 == int(re.search(r"#define MMHN_ABI_VERSION (\d+)", hdr).group(1))


@pytest.mark.gpu
@pytest.mark.parametrize("e", [e for e in ENTRIES.values() if e.luad], ids=lambda e: e.cohort)
def test_bitwise_reproducible_and_batching(e, golden):
    """The rows of LUAD-28 twice, then in another order through a small workspace.  (sample_orders, whose samples depend
    on the index of their row, has test_reproducible_whatever_the_call of its own.)"""
    from metmhn_amd.engine import Engine
    from metmhn_amd.jx import engine
    prefix, select = e.luad
    mod, dat = luad(golden, prefix)
    dat = dat[select(dat)]
    k = dat[:, :-2].astype(int).sum(1)
    args = (mod.log_theta, mod.obs1, mod.obs2)
    first = getattr(engine(mod.n), e.engine)(*args, dat)
    again = getattr(engine(mod.n), e.engine)(*args, dat)
    for x, y in zip(first, again):
        np.testing.assert_array_equal(x, y)
    keep = np.flatnonzero(k <= 16)
    assert k[keep].max() == 16 and (k[keep] >= 15).any()
    perm = np.random.default_rng(5).permutation(keep)
    with Engine(mod.n, workspace_bytes=8 << 20) as small:          # a k = 16 paired row needs 4.8 MiB: many batches
        b = getattr(small, e.engine)(*args, dat[perm])
        for x, y in zip(first, b):
            np.testing.assert_array_equal(x[perm], y)
        # a lattice larger than the whole workspace is turned away per row, the rest of the call goes on
        big = np.flatnonzero((dat[:, -1] == 3) & (k == 18))[:1]
        assert len(big) == 1
        *out, status = getattr(small, e.engine)(*args, np.vstack((dat[big], dat[keep[:5]])))
        assert status[0] == 3 and np.all(status[1:] == 0)
        for x, y in zip(first, out):
            assert np.all(np.isnan(y[0]))
            np.testing.assert_array_equal(y[1:], x[keep[:5]])
    print(f"bitwise: {len(dat)} rows twice, {len(perm)} permuted rows in batches of 8 MiB, one row turned away")
