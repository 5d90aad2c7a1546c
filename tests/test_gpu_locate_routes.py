"""GPU tests of one codec going through every locate route in turn.  The list
locates (rs_locate_dev_batch, rs_locate_set_dev_batch and the checked
rebuild's) share one pass body and the same three scratch buffers (scrub.cpp
pass_setup / scan_pass / locate_rounds), sized per call: here one codec object
runs them one after the other, with passes of different sizes and with a
larger shard size behind a smaller one, and every call must give the verdicts
its tampering calls for and leave the bytes a fresh codec leaves for that call
alone.  Built from the helpers of tests/test_gpu_scrub_set.py and
tests/test_gpu_checked.py; every expectation comes from the tampering and the
oracle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from tests import test_gpu_checked as chk
from tests import test_gpu_scrub_set as sset
from tests.test_gpu_scrub_set import FILL, NS, padded

pytestmark = pytest.mark.gpu

CLEAN, UNLOCATED = rs.SCRUB_CLEAN, rs.SCRUB_UNLOCATED
MAXS = rs.LOCATE_SET_MAX


def one_shard(want):
    """The one-shard routes' verdicts for tests.test_gpu_scrub_set.tamper's
    stripes: the shard where exactly one is corrupt.  Where t >= 2 shards are
    (t <= 5 here), replacing one shard cannot give a codeword, which would lie
    within t + 1 <= 6 shards of the untampered one, closer than the code's
    distance p + 1 (10 and 29 here): unlocated.  (Every data shard of both
    geometries has a ratio of its own, so a single corrupt one is named.)"""
    return [CLEAN if w == [] else w[0] if w is not None and len(w) == 1 else UNLOCATED for w in want]


def routes(bits, k, p, S):
    """The six calls of a sequence: (name, scrub_chunk, content of the slab,
    call(codec, slab) -> verdicts as lists, the verdicts expected)."""
    _, bad, want = sset.tamper(bits, k, p, S)
    _, cbad, missing, corrupt = chk.tamper(bits, k, p, S)
    table = chk.table_of(k, p, missing)
    centry = chk.prefill(cbad, missing, 1)
    cwant = chk.expected(bits, k, p, missing, corrupt)
    # stripe 8 has nothing missing and two corrupt data shards, within the cap of both geometries here
    assert missing[8] == [] and len(corrupt[8]) == 2 and sset.cap_of(bits, k, p) >= 2
    cwant[8] = list(corrupt[8])
    assert any(w for z, w in enumerate(cwant) if z != 8), "no degraded bad stripe is located"

    def both(r):
        return r[0].tolist(), r[1].tolist()

    def locate_set(c, slab):
        return both(c.locate_set_dev_batch(slab, range(NS), repair=True))

    return [
        ("locate_set", 1, bad, locate_set, sset.as_arrays(want, range(NS))),
        ("checked", 0, centry, lambda c, slab: both(c.reconstruct_checked_dev_batch_patterns(slab, table, range(NS), repair=True)),
         chk.as_arrays(cwant)),
        ("locate", 5, bad, lambda c, slab: c.locate_dev_batch(slab, range(NS), repair=True).tolist(), one_shard(want)),
        ("scrub_set", 0, bad, lambda c, slab: both(c.scrub_set_dev_batch(slab, repair=True)), sset.as_arrays(want, range(NS))),
        ("scrub", 0, bad, lambda c, slab: c.scrub_dev_batch(slab, repair=True).tolist(), one_shard(want)),
        ("locate_set again", 1, bad, locate_set, sset.as_arrays(want, range(NS))),
    ]


def run_sequence(bits, k, p, sizes, paths):
    c = rs.ReedSolomon(k, p, bits)
    for S in sizes:
        for name, chunk, content, call, expect in routes(bits, k, p, S):
            paths("scrub_chunk", chunk)
            backing, slab = padded(content)
            got = call(c, slab)
            assert got == expect, f"{name} at S = {S}"
            left = backing.cpu().numpy()
            assert (left[:, :, S:] == FILL).all(), f"{name} at S = {S}: padding bytes written"
            alone_backing, alone = padded(content)
            assert call(rs.ReedSolomon(k, p, bits), alone) == expect, f"{name} at S = {S}, a fresh codec"
            assert np.array_equal(left, alone_backing.cpu().numpy()), f"{name} at S = {S}: not the bytes of the call alone"


def test_every_route_on_one_codec_growing_buffers(paths):
    """GF(2^16) 37+9 (cap 4): S = 192, then S = 4160 on the same codec, whose
    slot and result buffers must grow."""
    run_sequence(16, 37, 9, (192, 4160), paths)


def test_every_route_on_one_codec_gf8(paths):
    """GF(2^8) 100+28: the other field, and the other piece size of the column sets."""
    run_sequence(8, 100, 28, (192,), paths)


def test_cap_one_takes_the_one_shard_route():
    """GF(2^16) 5+3 has cap 1 (p / 2): rs_locate_set_dev_batch hands the list to
    the one-shard route and re-encodes its verdicts.  (The scrub-set tests run
    2+1 through this call, where p = 1 locates nothing; this geometry locates.)
    Two corrupt shards are unlocated by the code's distance 4: one replaced
    shard cannot give a codeword 3 shards from another."""
    bits, k, p, S = 16, 5, 3, 64
    good = sset.stripes(bits, k, p, S, n=4)
    bad = np.array(good)
    bad[1, 2, 17] ^= 0x40
    bad[2, k + 1, 40] ^= 0x01
    bad[3, 0, 3] ^= 0x08
    bad[3, 4, 50] ^= 0x80
    c = rs.ReedSolomon(k, p, bits)
    backing, slab = padded(bad)
    before = backing.clone()
    count, shards = c.locate_set_dev_batch(slab, range(4), max_shards=4)
    assert count.tolist() == [0, 1, 1, UNLOCATED]
    assert shards.tolist() == [[-1] * 4, [2, -1, -1, -1], [k + 1, -1, -1, -1], [-1] * 4]
    v = c.locate_dev_batch(slab, range(4))
    assert v.tolist() == [CLEAN, 2, k + 1, UNLOCATED]
    assert shards[:, 0].tolist() == [x if x >= 0 else -1 for x in v.tolist()]
    assert torch.equal(backing, before), "repair=0 wrote something"


def stats(name):
    out = (C.c_uint64 * 3)()
    assert getattr(rs.lib(), name)(out, 1) == 0
    return [int(x) for x in out]


def test_the_two_routes_count_apart(paths):
    """rs_debug_locate_set_stats counts the set locate's passes, rounds and
    waits and rs_debug_checked_stats the checked locate's, though both run
    the same loop.  37+9: cap 4."""
    bits, k, p, S = 16, 37, 9, 192
    good, cbad, missing, corrupt = chk.tamper(bits, k, p, S)
    _, bad, _ = sset.tamper(bits, k, p, S)
    table = chk.table_of(k, p, missing)
    c = rs.ReedSolomon(k, p, bits)
    paths("scrub_chunk", 0)
    stats("rs_debug_locate_set_stats"), stats("rs_debug_checked_stats")
    # every bad stripe degraded: stripe 8, the one with nothing missing, is clean here
    degraded = np.array(cbad)
    degraded[8] = good[8]
    _, slab = padded(chk.prefill(degraded, missing, 1))
    count, _ = c.reconstruct_checked_dev_batch_patterns(slab, table, range(NS), repair=True)
    assert count[8] == 0 and (count != 0).any()
    assert stats("rs_debug_locate_set_stats") == [0, 0, 0]
    assert stats("rs_debug_checked_stats")[0] == 1
    # the set locate alone
    _, slab = padded(bad)
    c.locate_set_dev_batch(slab, range(NS), repair=True)
    assert stats("rs_debug_checked_stats") == [0, 0, 0]
    assert stats("rs_debug_locate_set_stats")[0] == 1
    # full and degraded bad stripes in one checked call: one pass of each
    _, slab = padded(chk.prefill(cbad, missing, 1))
    count, _ = c.reconstruct_checked_dev_batch_patterns(slab, table, range(NS), repair=True)
    assert count[8] == 2
    for name in ("rs_debug_locate_set_stats", "rs_debug_checked_stats"):
        passes, rounds, waits = stats(name)
        assert passes == 1 and 1 <= rounds <= MAXS and waits <= 1 + 2 * MAXS, name
