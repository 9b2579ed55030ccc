"""Philox4x32-10 in NumPy: the counter-based generator of metmhn_amd/csrc/sampler.h (`philox4x32_10`), for the host code
that must draw what a kernel draws (MetMHN.sample_order).  Words travel as uint64 arrays that hold 32-bit values, so that
the 32 x 32 -> 64 bit products do not overflow."""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_BUMP0, _BUMP1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays of 32-bit values) of the counter (c0, c1, c2, c3) under the key (k0, k1);
    the arguments broadcast against each other."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _BUMP0) & _M32, (k1 + _BUMP1) & _M32
    return c0, c1, c2, c3


def uniform53(r0, r1):
    """gillespie_step's uniform in [0, 1): the top 27 bits of r0 and the top 26 of r1 as a 53-bit fraction."""
    m = ((np.asarray(r0, dtype=np.uint64) >> np.uint64(5)) << np.uint64(26)) | (np.asarray(r1, dtype=np.uint64) >> np.uint64(6))
    return m.astype(np.float64) * (1.0 / 9007199254740992.0)


def order_uniforms(seed: int, row: int, samples, move: int):
    """The uniform of move number `move` of the order samples `samples` (uint64 sample indices) of cohort row `row`:
    key = the 64-bit seed, counter = (sample low word, sample high word, move, row + 1) - word 3 = 0 is the Gillespie
    sampler's stream."""
    seed = int(seed) & (2 ** 64 - 1)
    s = np.asarray(samples, dtype=np.uint64)
    r0, r1, _, _ = philox4x32_10(s & _M32, s >> _S32, np.uint64(move), np.uint64((int(row) + 1) & 0xFFFFFFFF),
                                 np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    return uniform53(r0, r1)
