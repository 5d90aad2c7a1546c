"""Helpers shared by tests/test_checked_cpu.py and tests/test_gpu_checked.py:
filling a degraded stripe with the numpy oracle (which, like the reference,
rebuilds from all survivors), the syndrome rows of the filled stripe, and the
brute-force statement "no set of at most t survivors explains this degraded
stripe" (tests/scrub_set_util.explains with the missing rows added).
"""
import itertools

import numpy as np

from oracle import leopard_np, orc
from tests.scrub_set_util import explains


def codeword(bits, k, p, S, seed):
    rng = np.random.default_rng(seed)
    stripe = np.empty((k + p, S), np.uint8)
    stripe[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
    stripe[k:] = orc.encode(bits, k, p, stripe[:k])
    return stripe, rng


def fill(bits, k, p, stripe, missing, numpy_oracle=True):
    """`stripe` with the rows `missing` replaced by what the oracle's
    reconstruct gives from all the others."""
    out = np.array(stripe)
    if not len(missing):
        return out
    shards = [None if i in missing else np.ascontiguousarray(stripe[i]) for i in range(k + p)]
    if numpy_oracle:
        for i, row in leopard_np.reconstruct(bits, k, p, shards, recover_all=True).items():
            out[i] = row
    else:
        err, rows = orc.Oracle(bits, k, p).reconstruct(shards, recover_all=True)
        assert err == 0, err
        for i in missing:
            out[i] = rows[i]
    return out


def syndrome(bits, k, p, filled):
    """e_i = P_i ^ P'_i of a complete stripe, as symbols [p, nsym]."""
    fresh = orc.encode(bits, k, p, np.ascontiguousarray(filled[:k]))
    return leopard_np.to_symbols(fresh, bits) ^ leopard_np.to_symbols(np.ascontiguousarray(filled[k:]), bits)


def explaining_survivor_sets(bits, k, p, stripe, missing, t):
    """Every set of exactly t survivors whose removal (with the missing rows)
    leaves rows that the oracle completes to a codeword agreeing with them."""
    missing = set(int(x) for x in missing)
    alive = [i for i in range(k + p) if i not in missing]
    if k + p - len(missing) - t < k:
        return []
    return [J for J in itertools.combinations(alive, t) if explains(bits, k, p, stripe, missing | set(J))]
