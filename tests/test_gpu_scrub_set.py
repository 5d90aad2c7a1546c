"""GPU tests of the set locate (rs_locate_set_dev_batch, rs_scrub_set_dev_batch;
stream_kernels.hip k_syndrome_pick_rows, k_syndrome_confirm_set, k_syndrome_fix_set)
on oracle-encoded stripes in a padded slab: every listed stripe gets exactly
the set of shards that was tampered with, a located set is repaired bit for
bit, and nothing else -- padding, clean stripes, unlocated stripes, corrupt
stripes that are not listed -- is written.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc
from tests.scrub_set_util import explaining_sets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS, PAD, FILL = 12, 64, 0xA5
CLEAN, UNLOCATED = rs.SCRUB_CLEAN, rs.SCRUB_UNLOCATED
MAXS = rs.LOCATE_SET_MAX
SKIPPED = 10  # a corrupt stripe the lists of test_repair_* leave out

# 64: one block; 192: an odd block count; 4160: more than one workgroup
ALL = (64, 192, 4160)
# tests/test_gpu_scrub_batch.py's nine geometries, one per verify path, then
# 12+7 (with 37+9: sets of 3 and 4, p < m, the shift a = p)
GEOMS = [
    (16, 128, 32, ALL, {}),
    (16, 37, 9, ALL, {}),
    (16, 10, 4, ALL, {}),
    (16, 3, 7, ALL, {}),
    (16, 2, 1, ALL, {}),
    (16, 200, 100, (64, 192), {}),
    (8, 10, 4, ALL, {}),
    (8, 128, 128, ALL, {}),
    (16, 600, 300, (64,), {"lds_big": 0}),
    (16, 12, 7, ALL, {}),
]
CASES = [pytest.param(b, k, p, S, knobs, id=f"{b}-{k}+{p}-S{S}") for b, k, p, sizes, knobs in GEOMS for S in sizes]

_slabs, _tampered = {}, {}


def cap_of(bits, k, p):
    m = 1 << max(p - 1, 0).bit_length()
    shift = p < m or m + k < (1 << bits)
    return max(1, min(MAXS, p // 2)) if shift else 1


def stripes(bits, k, p, S, n=NS):
    """n oracle-encoded stripes [n, k+p, S] for a geometry and size, computed once and never written."""
    key = (bits, k, p, S, n)
    if key not in _slabs:
        rng = np.random.default_rng(bits * 6151 + k * 131 + p * 17 + S + n)
        out = np.empty((n, k + p, S), np.uint8)
        for z in range(n):
            out[z, :k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
            out[z, k:] = orc.encode(bits, k, p, out[z, :k])
        out.setflags(write=False)
        _slabs[key] = out
    return _slabs[key]


def padded(content):
    n, rows, S = content.shape
    host = np.full((n, rows, S + PAD), FILL, np.uint8)
    host[:, :, :S] = content
    backing = torch.from_numpy(host).to(DEV)
    slab = backing[:, :, :S]
    assert slab.stride(1) == S + PAD
    return backing, slab


def codec(bits, k, p, knobs, paths):
    for knob, v in knobs.items():
        paths(knob, v)
    return rs.ReedSolomon(k, p, bits)


def tamper(bits, k, p, S):
    """(good, bad, expected sets): a copy of the stripes with, by stripe:
    0 two data shards in the same byte; 1 two data shards in disjoint places,
    one in the first 64-byte block only and one in the last only (the first
    decode names one shard, the confirm fails, a second round finds the other);
    2 a data and a parity shard; 3 parity shards 0 and 1; 4 a high-byte half in
    one shard and the low-byte half 32 below it in another; 5 two whole rows of
    random bytes; 6 cap shards, data and parity, in a common byte and in bytes
    of their own; 7 cap + 1 whole rows of random bytes: no set of at most cap
    shards explains them (2 cap + 1 <= p: by the code's distance; p = 4: by
    brute force with the numpy oracle, as tests/test_scrub_set_cpu.py does); 8
    one data shard; 9 clean; 10 two data shards (the stripe the lists leave
    out); 11 clean.  An expected entry is the sorted list of shards, [] for
    clean, None for unlocated."""
    key = (bits, k, p, S)
    if key in _tampered:
        return _tampered[key]
    good = stripes(bits, k, p, S)
    cap = cap_of(bits, k, p)
    rng = np.random.default_rng(k * 977 + p * 31 + S + bits)
    bad = np.array(good)
    want = [None] * NS

    def pair():
        return sorted(int(x) for x in rng.choice(k, 2, replace=False))

    def random_row(z, r):
        row = rng.integers(0, 256, S, dtype=np.uint8)
        row[7] = good[z, r, 7] ^ 0x80  # (certainly another row)
        bad[z, r] = row

    def located(J):
        J = sorted(set(J))
        if p == 1 or len(J) > cap:
            return None
        return J

    a, b = pair()
    bad[0, a, 5] ^= 0x10
    bad[0, b, 5] ^= 0x03
    want[0] = located([a, b])
    a, b = pair()
    bad[1, a, 3] ^= 0x20
    bad[1, b, S - 2] ^= 0x02
    want[1] = located([a, b])
    a = int(rng.integers(0, k))
    bad[2, a, 9] ^= 0x11
    bad[2, k + p - 1, 9] ^= 0x01
    want[2] = located([a, k + p - 1])
    bad[3, k, S // 2] ^= 0x04
    bad[3, k + min(p - 1, 1), S - 1] ^= 0x80
    want[3] = located([k, k + min(p - 1, 1)])
    a, b = pair()
    bad[4, a, S - 64 + 32 + 5] ^= 0x08
    bad[4, b, S - 64 + 5] ^= 0x40
    want[4] = located([a, b])
    a = int(rng.integers(0, k))
    pi = int(rng.integers(0, p))
    random_row(5, a)
    random_row(5, k + pi)
    want[5] = located([a, k + pi])
    J = sorted(int(x) for x in rng.choice(k + p, cap, replace=False))
    for t, x in enumerate(J):
        bad[6, x, 20] ^= 1 + t
        bad[6, x, (11 * t + 1) % S] ^= 0x80
    want[6] = located(J)
    over = sorted(int(x) for x in rng.choice(k + p, cap + 1, replace=False))
    for x in over:
        random_row(7, x)
    if p == 4 and cap == 2:
        assert explaining_sets(bits, k, p, bad[7], 2) == [], "pick another seed: a pair explains three random rows"
    else:
        assert cap == 1 or 2 * cap + 1 <= p
    a = int(rng.integers(0, k))
    bad[8, a, S - 1] ^= 0x01
    want[8] = located([a])
    want[9] = []
    a, b = pair()
    bad[10, a, 1] ^= 0x40
    bad[10, b, 2] ^= 0x40
    want[10] = located([a, b])
    want[11] = []
    bad.setflags(write=False)
    _tampered[key] = (good, bad, want)
    return _tampered[key]


def as_arrays(want, lst, ms=MAXS):
    count = [UNLOCATED if want[z] is None else len(want[z]) for z in lst]
    shards = [([] if want[z] is None else want[z]) + [-1] * ms for z in lst]
    return count, [row[:ms] for row in shards]


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_sets_are_located(bits, k, p, S, knobs, paths):
    good, bad, want = tamper(bits, k, p, S)
    c = codec(bits, k, p, knobs, paths)
    backing, slab = padded(bad)
    before = backing.clone()
    count, shards = c.locate_set_dev_batch(slab, range(NS))
    wc, ws = as_arrays(want, range(NS))
    assert count.dtype == np.int32 and shards.dtype == np.int32 and shards.shape == (NS, MAXS)
    assert count.tolist() == wc
    assert shards.tolist() == ws
    assert torch.equal(backing, before), "repair=0 wrote something"
    # max_shards = 1 is rs_locate_dev_batch, re-encoded
    v = c.locate_dev_batch(slab, range(NS))
    c1, s1 = c.locate_set_dev_batch(slab, range(NS), max_shards=1)
    assert c1.tolist() == [0 if x == CLEAN else 1 if x >= 0 else UNLOCATED for x in v]
    assert s1[:, 0].tolist() == [x if x >= 0 else -1 for x in v]
    # the stripe with one corrupt shard: both calls agree
    assert count[8] == c1[8] and shards[8, 0] == s1[8, 0] == max(int(v[8]), -1) and (shards[8, 1:] == -1).all()
    # a smaller max_shards: the sets that fit are the same, the others are unlocated
    c2, s2 = c.locate_set_dev_batch(slab, range(NS), max_shards=2)
    for z in range(NS):
        fits = want[z] is not None and len(want[z]) <= 2
        assert c2[z] == (len(want[z]) if fits else UNLOCATED), f"stripe {z}"
        assert s2[z].tolist() == ((want[z] + [-1, -1])[:2] if fits else [-1, -1])
    # clean stripes only, and an empty list
    assert c.locate_set_dev_batch(slab, [11, 9])[0].tolist() == [0, 0]
    assert c.locate_set_dev_batch(slab, [])[0].tolist() == []
    assert torch.equal(backing, before)


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_repair_shuffled_list_in_chunks(bits, k, p, S, knobs, paths):
    """A shuffled list without stripe SKIPPED, in passes of 1, of 5 and of the
    automatic size: equal results, the located sets restored bit for bit, the
    unlocated and the unlisted stripes and the padding as they were, a second
    call clean."""
    good, bad, want = tamper(bits, k, p, S)
    c = codec(bits, k, p, knobs, paths)
    rng = np.random.default_rng(S + k)
    lst = [int(z) for z in rng.permutation(NS) if z != SKIPPED]
    wc, ws = as_arrays(want, lst)
    results = []
    for chunk in (1, 5, 0):
        paths("scrub_chunk", chunk)
        backing, slab = padded(bad)
        count, shards = c.locate_set_dev_batch(slab, lst, repair=True)
        assert count.tolist() == wc and shards.tolist() == ws, f"chunk {chunk}"
        got = backing.cpu().numpy()
        assert (got[:, :, S:] == FILL).all(), "padding bytes written"
        for z in range(NS):
            fixed = z != SKIPPED and want[z] is not None
            assert np.array_equal(got[z, :, :S], good[z] if fixed else bad[z]), f"chunk {chunk} stripe {z}"
        again, sh = c.locate_set_dev_batch(slab, lst, repair=True)
        assert again.tolist() == [UNLOCATED if want[z] is None else 0 for z in lst]
        assert (sh == -1).all()
        assert np.array_equal(backing.cpu().numpy(), got), "the second call wrote something"
        results.append(got)
    assert all(np.array_equal(results[0], r) for r in results[1:])


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_scrub_set_is_the_map_and_the_list_call(bits, k, p, S, knobs, paths):
    good, bad, want = tamper(bits, k, p, S)
    c = codec(bits, k, p, knobs, paths)
    backing, slab = padded(bad)
    before = backing.clone()
    flags = c.verify_dev_batch_map(slab)
    lst = [z for z in range(NS) if flags[z]]
    assert lst == [z for z in range(NS) if want[z] != []]
    lc, ls = c.locate_set_dev_batch(slab, lst)
    count = np.full(NS, 77, np.int32)
    shards = np.full((NS, 3), 77, np.int32)
    nbad = C.c_int(-1)
    for repair in (0, 1):
        e = c._L.rs_scrub_set_dev_batch(c._h, slab.data_ptr(), slab.stride(1), slab.stride(0), NS, S, 3, repair,
                                        count.ctypes.data, shards.ctypes.data, C.byref(nbad), None)
        assert e == 0 and nbad.value == len(lst)
        for z in range(NS):
            fits = want[z] is not None and len(want[z]) <= 3
            assert count[z] == (len(want[z]) if fits else UNLOCATED), f"stripe {z}"
            assert shards[z].tolist() == ((want[z] + [-1] * 3)[:3] if fits else [-1] * 3)
        if not repair:
            assert torch.equal(backing, before), "repair=0 wrote something"
    for i, z in enumerate(lst):  # the list call with max_shards = 4 names the same sets
        assert lc[i] == (UNLOCATED if want[z] is None else len(want[z])) and ls[i].tolist() == as_arrays(want, [z])[1][0]
    got = backing.cpu().numpy()
    for z in range(NS):
        fixed = want[z] is not None and len(want[z]) <= 3
        assert np.array_equal(got[z, :, :S], good[z] if fixed else bad[z]), f"stripe {z}"
    assert (got[:, :, S:] == FILL).all(), "padding bytes written"
    mc, ms = c.scrub_set_dev_batch(slab)
    assert mc.tolist() == [0 if (want[z] is not None and len(want[z]) <= 3) else (UNLOCATED if want[z] is None else len(want[z]))
                           for z in range(NS)]


@pytest.mark.parametrize("null_stream", [False, True])
def test_locate_set_is_stream_ordered(null_stream, paths):
    """The corruption is a torch op on the stream and the call is queued right
    behind it: no synchronise in between."""
    bits, k, p, S = 16, 37, 9, 4160
    good = stripes(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    paths("scrub_chunk", 2)
    backing, slab = padded(good)
    mask = torch.zeros(S, dtype=torch.uint8, device=DEV)
    mask[100:164] = 0x5A
    mask2 = torch.zeros(S, dtype=torch.uint8, device=DEV)
    mask2[4000:4100] = 0xC3
    torch.cuda.synchronize()
    st = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    with torch.cuda.stream(st):
        slab[2, 11] ^= mask
        slab[2, 30] ^= mask2
        slab[3, k + 4] ^= mask
        slab[3, 0] ^= mask
        slab[3, k] ^= mask2
        slab[7, 36] ^= mask
        count, shards = c.locate_set_dev_batch(slab, [7, 0, 3, 2, 11], repair=True, stream=st)
        ok = c.verify_dev_batch(slab, stream=st)
    assert count.tolist() == [1, 0, 3, 2, 0]
    assert shards.tolist() == [[36, -1, -1, -1], [-1] * 4, [0, k, k + 4, -1], [11, 30, -1, -1], [-1] * 4]
    assert ok
    assert np.array_equal(slab.cpu().numpy(), good)
    assert bool((backing[:, :, S:] == FILL).all())


def route_stats(reset=True):
    out = (C.c_uint64 * 3)()
    assert rs.lib().rs_debug_locate_set_stats(out, int(reset)) == 0
    return [int(x) for x in out]


@pytest.mark.parametrize("chunk", [0, 5, 1])
def test_rounds_and_host_waits_are_bounded(chunk, paths):
    """Per pass at most cap confirm rounds and 1 + 2 cap host waits, however
    many stripes the pass holds (rs_debug_locate_set_stats).  37+9: cap 4."""
    bits, k, p, S = 16, 37, 9, 192
    good, bad, want = tamper(bits, k, p, S)
    cap = cap_of(bits, k, p)
    c = rs.ReedSolomon(k, p, bits)
    paths("scrub_chunk", chunk)
    backing, slab = padded(bad)
    assert rs.lib().rs_debug_locate_set_stats(None, 0) != 0
    route_stats()
    count, _ = c.locate_set_dev_batch(slab, range(NS))
    passes, rounds, waits = route_stats()
    assert count.tolist() == as_arrays(want, range(NS))[0]
    assert passes == (1 if chunk == 0 else -(-NS // chunk))
    assert rounds <= cap * passes and waits <= (1 + 2 * cap) * passes
    # stripe 1 (two shards in disjoint places) needs a second round wherever it sits
    assert rounds >= 2
    if chunk == 0:
        assert waits >= 1 + 2 * 2
    assert route_stats() == [0, 0, 0], "the read with reset clears the counters"
    # one pass over stripe 0 alone (two shards in one byte): the scan, one pick, one confirm
    c.locate_set_dev_batch(slab, [0])
    assert route_stats() == [1, 1, 3]
    # ... and over stripe 1 alone: a second pick and a second confirm
    c.locate_set_dev_batch(slab, [1])
    assert route_stats() == [1, 2, 5]
    # a clean stripe takes the scan's wait only; cap 1 does not take this route at all
    c.locate_set_dev_batch(slab, [9])
    assert route_stats() == [1, 0, 1]
    c.locate_set_dev_batch(slab, range(NS), max_shards=1)
    assert route_stats() == [0, 0, 0]


def test_pairs_in_more_columns_than_one_column_set():
    """12+32768: a column's tables take 3 MiB, so the 32 MiB table bound holds 8
    columns; six stripes bad in the data shards (2 z, 2 z + 1) have twelve
    distinct columns and are confirmed (and repaired) in more than one piece.
    A seventh stripe is clean."""
    bits, k, p, S, n = 16, 12, 32768, 64, 7
    rng = np.random.default_rng(12 + 32768 + 2)
    one = np.empty((k + p, S), np.uint8)
    one[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
    one[k:] = orc.encode(bits, k, p, one[:k])
    good = np.repeat(one[None], n, axis=0)
    bad = good.copy()
    for z in range(6):
        bad[z, 2 * z, 5 * z] ^= 0x21
        bad[z, 2 * z + 1, 5 * z + (z % 2)] ^= 0x07  # the same symbol, or the next
    want = [[2 * z, 2 * z + 1, -1, -1] for z in range(6)] + [[-1] * 4]
    c = rs.ReedSolomon(k, p, bits)
    backing, slab = padded(bad)
    count, shards = c.locate_set_dev_batch(slab, range(n))
    assert count.tolist() == [2] * 6 + [0] and shards.tolist() == want
    count, shards = c.locate_set_dev_batch(slab, range(n), repair=True)
    assert count.tolist() == [2] * 6 + [0] and shards.tolist() == want
    got = backing.cpu().numpy()
    assert np.array_equal(got[:, :, :S], good)
    assert (got[:, :, S:] == FILL).all()
