"""Helpers shared by tests/test_scrub_set_cpu.py and tests/test_gpu_scrub_set.py:
the field product on numpy arrays, and the brute-force statement "no set of
at most t shards explains this stripe", established with the numpy oracle
alone (reconstruct with the set erased, put the result in place, verify).
"""
import itertools

import numpy as np

from oracle import leopard_np


def gf_mul(bits, a, b):
    """Element-wise product of two symbol arrays."""
    F = leopard_np.field(bits)
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    r = F._exp[F.add_mod(F._log[a], F._log[b])]
    return np.where((a == 0) | (b == 0), 0, r)


def explains(bits, k, p, stripe, J):
    """True when replacing the shards J of `stripe` ([k+p, S] bytes) by what the
    oracle reconstructs from the others gives a codeword."""
    shards = [None if i in J else stripe[i] for i in range(k + p)]
    rebuilt = leopard_np.reconstruct(bits, k, p, shards, recover_all=True)
    fixed = np.array(stripe)
    for i, row in rebuilt.items():
        fixed[i] = row
    return np.array_equal(leopard_np.encode(bits, k, p, fixed[:k]), fixed[k:])


def explaining_sets(bits, k, p, stripe, t):
    """Every set of exactly t shards that explains the stripe."""
    return [J for J in itertools.combinations(range(k + p), t) if explains(bits, k, p, stripe, set(J))]


def over_capacity_stripe(bits, k, p, S, nrows, seed):
    """An oracle-encoded stripe with nrows whole rows replaced by seeded random
    bytes: (good, bad, the rows)."""
    rng = np.random.default_rng(seed)
    good = np.empty((k + p, S), np.uint8)
    good[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
    good[k:] = leopard_np.encode(bits, k, p, good[:k])
    rows = sorted(int(x) for x in rng.choice(k + p, nrows, replace=False))
    bad = good.copy()
    for r in rows:
        bad[r] = rng.integers(0, 256, S, dtype=np.uint8)
        bad[r, 0] = good[r, 0] ^ 0x5A  # certainly another row
    return good, bad, rows
