"""GPU tests of the checked rebuild (rs_reconstruct_checked_dev_batch_patterns;
stream_kernels.hip k_syndrome_fix_present, with k_syndrome_confirm_set on the check
matrix's columns) on oracle-encoded stripes in a padded slab, one erasure
pattern per stripe: every stripe gets exactly the verdict its tampering calls
for, a located stripe ends bit for bit as the codeword, and everything else is
what rs_reconstruct_dev_batch_patterns alone leaves.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from tests.test_gpu_scrub_set import ALL, DEV, FILL, NS, codec, padded, stripes

pytestmark = pytest.mark.gpu

UNLOCATED = rs.SCRUB_UNLOCATED
MAXS = rs.LOCATE_SET_MAX

GEOMS = [
    (16, 128, 32, ALL, {}),  # the bit-sliced decoder
    (16, 37, 9, ALL, {}),
    (16, 12, 7, ALL, {}),
    (16, 10, 4, ALL, {}),
    (16, 2, 1, ALL, {}),
    (16, 200, 100, (64, 192), {}),
    (16, 600, 300, (64,), {"lds_big": 0}),
    (8, 10, 4, ALL, {}),
    (8, 100, 28, ALL, {}),
    (8, 128, 128, ALL, {}),  # no shift point
]
CASES = [pytest.param(b, k, p, S, knobs, id=f"{b}-{k}+{p}-S{S}") for b, k, p, sizes, knobs in GEOMS for S in sizes]

_tampered = {}


def has_shift(bits, k, p):
    m = 1 << max(p - 1, 0).bit_length()
    return p < m or m + k < (1 << bits)


def cap_z(p, e, ms=MAXS):
    return min(ms, (p - e) // 2)


def tamper(bits, k, p, S):
    """(good, bad, missing, corrupt): a copy of the stripes with, by stripe, the
    rows `missing[z]` marked missing and the survivors `corrupt[z]` damaged:
    0 one row missing, clean; 1 one row missing, one corrupt data survivor; 2 e
    rows missing and cap_z corrupt survivors, data and parity, sharing one byte;
    3 the same in disjoint 64-byte blocks, the first and the last; 4 parity
    shard 0 missing and a corrupt parity survivor; 5 p - 1 rows missing and a
    corrupt survivor; 6 p rows missing and a corrupt survivor; 7 one row missing
    and cap_z + 1 whole random rows where 2 (cap_z + 1) + 1 <= p (else clean);
    8 nothing missing, two corrupt data shards; 9 nothing missing, clean; 10 a
    high-byte half in one survivor and the low-byte half 32 below it in
    another, one row missing; 11 clean with p / 2 rows missing."""
    key = (bits, k, p, S)
    if key in _tampered:
        return _tampered[key]
    good = stripes(bits, k, p, S)
    rng = np.random.default_rng(k * 1009 + p * 37 + S + bits + 5)
    n = k + p
    bad = np.array(good)
    missing = [[] for _ in range(NS)]
    corrupt = [[] for _ in range(NS)]

    def pick(z, e, must=()):
        rest = [i for i in range(n) if i not in must]
        missing[z] = sorted(list(must) + [int(x) for x in rng.choice(rest, e - len(must), replace=False)])

    def survivors(z, count, data=None):
        alive = [i for i in range(n) if i not in missing[z] and (data is None or (i < k) == data)]
        return sorted(int(x) for x in rng.choice(alive, count, replace=False))

    pick(0, 1)
    pick(1, 1)
    corrupt[1] = survivors(1, 1, data=True)
    bad[1, corrupt[1][0], 9] ^= 0x10
    e2 = min(max(p - 2, 1), max(1, p // 3))
    for z in (2, 3):
        pick(z, e2)
        c = cap_z(p, e2)
        if c >= 2:
            corrupt[z] = sorted(survivors(z, 1, data=True) + survivors(z, c - 1, data=False))
        elif c == 1:
            corrupt[z] = survivors(z, 1)
        elif e2 < p:
            corrupt[z] = survivors(z, 1)  # detected, cap_z = 0
    for t, x in enumerate(corrupt[2]):
        bad[2, x, 20] ^= 1 + t
    for t, x in enumerate(corrupt[3]):
        bad[3, x, 3 if t == 0 else S - 2 - t] ^= 0x20 + t
    pick(4, 1, must=(k,))
    if p >= 2:
        corrupt[4] = [k + 1]
        bad[4, k + 1, S - 1] ^= 0x80
    if p >= 2:
        pick(5, p - 1)
    corrupt[5] = survivors(5, 1, data=True)
    bad[5, corrupt[5][0], 11] ^= 0x04
    pick(6, p)
    x = survivors(6, 1)[0]  # not listed in corrupt: with p rows missing nothing can tell
    bad[6, x, 13] ^= 0x40
    pick(7, 1)
    if 2 * (cap_z(p, 1) + 1) + 1 <= p:
        corrupt[7] = survivors(7, cap_z(p, 1) + 1)
        for x in corrupt[7]:
            row = rng.integers(0, 256, S, dtype=np.uint8)
            row[7] = good[7, x, 7] ^ 0x80  # (certainly another row)
            bad[7, x] = row
    if k >= 2:
        corrupt[8] = sorted(int(x) for x in rng.choice(k, 2, replace=False))
        bad[8, corrupt[8][0], 5] ^= 0x10
        bad[8, corrupt[8][1], 5] ^= 0x03
    pick(10, 1)
    if p >= 2:
        corrupt[10] = survivors(10, 2)
        bad[10, corrupt[10][0], S - 64 + 32 + 5] ^= 0x08
        bad[10, corrupt[10][1], S - 64 + 5] ^= 0x40
    if p >= 2:
        pick(11, p // 2)
    bad.setflags(write=False)
    _tampered[key] = (good, bad, missing, corrupt)
    return _tampered[key]


def expected(bits, k, p, missing, corrupt, ms=MAXS):
    """Per stripe with missing rows: [] consistent, the sorted set, or None for
    unlocated.  Every verdict is forced by the code's distance: a located set
    has |T| + cap_z <= p - e, an unlocated one |T| + cap_z + e <= p."""
    want = []
    for z in range(NS):
        e, T = len(missing[z]), corrupt[z]
        c = cap_z(p, e, ms)
        if e == p or not T:
            want.append([])
        elif has_shift(bits, k, p) and len(T) <= c:
            assert len(T) + c <= p - e
            want.append(list(T))
        else:
            assert c <= 0 or not has_shift(bits, k, p) or len(T) + c + e <= p
            want.append(None)
    return want


def table_of(k, p, missing):
    table = np.ones((NS, k + p), np.uint8)
    for z in range(NS):
        table[z, missing[z]] = 0
    return table


def prefill(content, missing, mode, seed=1):
    """The rows marked missing hold zeros or random bytes on entry."""
    out = np.array(content)
    rng = np.random.default_rng(seed)
    for z in range(NS):
        for r in missing[z]:
            out[z, r] = 0 if mode == 0 else rng.integers(0, 256, out.shape[2], dtype=np.uint8)
    return out


def as_arrays(want, ms=MAXS):
    w = max(ms, 1)
    count = [UNLOCATED if x is None else len(x) for x in want]
    shards = [(([] if x is None else x) + [-1] * w)[:w] for x in want]
    return count, shards


def rebuilt_only(c, content, table):
    """What rs_reconstruct_dev_batch_patterns leaves of a slab."""
    backing, slab = padded(content)
    c.reconstruct_dev_batch_patterns(slab, table, range(NS))
    torch.cuda.synchronize()
    return backing.cpu().numpy()


def scrub_set_only(c, content, ms, repair):
    backing, slab = padded(content)
    count, shards = c.scrub_set_dev_batch(slab, max_shards=ms, repair=repair)
    return count, shards, backing.cpu().numpy()


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_checked_rebuild(bits, k, p, S, knobs, paths):
    good, bad, missing, corrupt = tamper(bits, k, p, S)
    c = codec(bits, k, p, knobs, paths)
    table = table_of(k, p, missing)
    want = expected(bits, k, p, missing, corrupt)
    zero, rand = prefill(bad, missing, 0), prefill(bad, missing, 1)
    rec = rebuilt_only(c, zero, table)
    assert np.array_equal(rec, rebuilt_only(c, rand, table))
    # stripe 8 has nothing missing: rs_scrub_set_dev_batch's verdict and repair
    sc, ss, srep = scrub_set_only(c, bad, MAXS, True)
    wc, ws = as_arrays(want)
    wc[8], ws[8] = int(sc[8]), ss[8].tolist()

    # repair = 0: the verdicts, and exactly the plain rebuild's bytes
    backing, slab = padded(zero)
    count, shards = c.reconstruct_checked_dev_batch_patterns(slab, table, range(NS))
    assert count.dtype == np.int32 and shards.dtype == np.int32 and shards.shape == (NS, MAXS)
    assert count.tolist() == wc
    assert shards.tolist() == ws
    assert np.array_equal(backing.cpu().numpy(), rec), "repair=0 wrote more than the rebuild"

    # repair = 1, the missing rows zero or random on entry: the same verdicts and bytes
    results = []
    for content in (zero, rand):
        backing, slab = padded(content)
        count, shards = c.reconstruct_checked_dev_batch_patterns(slab, table, range(NS), repair=True)
        assert count.tolist() == wc and shards.tolist() == ws
        got = backing.cpu().numpy()
        assert (got[:, :, S:] == FILL).all(), "padding bytes written"
        for z in range(NS):
            if z == 8:
                assert np.array_equal(got[z], srep[z]), "nothing missing: rs_scrub_set_dev_batch's repair"
            elif want[z]:
                assert np.array_equal(got[z, :, :S], good[z]), f"stripe {z} is not the codeword"
            else:
                assert np.array_equal(got[z], rec[z]), f"stripe {z}: more than the rebuild was written"
        results.append(got)
    assert np.array_equal(results[0], results[1])

    # smaller max_shards: the sets that fit are the same, the others unlocated, nothing written
    for ms in (0, 1, 2):
        wm = expected(bits, k, p, missing, corrupt, ms)
        mc, msh = as_arrays(wm, ms)
        if ms:
            c8, s8, _ = scrub_set_only(c, bad, ms, False)
            mc[8], msh[8] = int(c8[8]), s8[8].tolist()
        else:
            mc[8], msh[8] = (UNLOCATED if corrupt[8] else 0), [-1]
        backing, slab = padded(rand)
        count, shards = c.reconstruct_checked_dev_batch_patterns(slab, table, range(NS), max_shards=ms)
        assert count.tolist() == mc, f"max_shards {ms}"
        assert shards.tolist() == msh, f"max_shards {ms}"
        assert np.array_equal(backing.cpu().numpy(), rec)


@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 4160), (16, 12, 7, 192), (8, 100, 28, 64), (8, 128, 128, 64)])
def test_clean_degraded_slab_is_the_plain_rebuild(bits, k, p, S):
    good, _, missing, _ = tamper(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    table = table_of(k, p, missing)
    content = prefill(good, missing, 1, seed=3)
    rec = rebuilt_only(c, content, table)
    assert np.array_equal(rec[:, :, :S], good)
    for repair in (False, True):
        backing, slab = padded(content)
        nbad = C.c_int(-1)
        count = np.full(NS, 77, np.int32)
        shards = np.full((NS, 3), 77, np.int32)
        of = np.arange(NS, dtype=np.uint32)
        e = c._L.rs_reconstruct_checked_dev_batch_patterns(
            c._h, slab.data_ptr(), slab.stride(1), slab.stride(0), NS, table.ctypes.data_as(C.POINTER(C.c_uint8)), NS,
            of.ctypes.data_as(C.POINTER(C.c_uint32)), S, 3, int(repair), count.ctypes.data, shards.ctypes.data,
            C.byref(nbad), None)
        assert e == 0 and nbad.value == 0
        assert (count == 0).all() and (shards == -1).all()
        assert np.array_equal(backing.cpu().numpy(), rec)


@pytest.mark.parametrize("null_stream", [False, True])
def test_checked_rebuild_is_stream_ordered(null_stream, paths):
    """The damage is a torch op on the stream and the call is queued right
    behind it: no synchronise in between."""
    bits, k, p, S = 16, 37, 9, 4160
    good = stripes(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    paths("scrub_chunk", 2)
    backing, slab = padded(good)
    table = np.ones((3, k + p), np.uint8)
    table[1, [4, k + 2]] = 0
    table[2, [0, 1, 2, k]] = 0
    of = [0, 1, 2, 1, 0, 2, 1, 1, 0, 0, 0, 0]
    mask = torch.zeros(S, dtype=torch.uint8, device=DEV)
    mask[100:164] = 0x5A
    mask2 = torch.zeros(S, dtype=torch.uint8, device=DEV)
    mask2[4000:4100] = 0xC3
    torch.cuda.synchronize()
    st = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    with torch.cuda.stream(st):
        slab[1, 4] = 0x11  # missing rows: anything
        slab[1, k + 2] = 0x22
        slab[1, 11] ^= mask
        slab[1, k + 5] ^= mask2
        slab[2, :3] = 0
        slab[2, k] = 0x33
        slab[2, 30] ^= mask
        slab[3, 4] = 0
        slab[3, k + 2] = 0
        slab[4, 7] ^= mask2
        count, shards = c.reconstruct_checked_dev_batch_patterns(slab, table, of, repair=True, stream=st)
        ok = c.verify_dev_batch(slab, stream=st)
    assert count.tolist() == [0, 2, 1, 0, 1] + [0] * 7
    assert shards[:5].tolist() == [[-1] * 4, [11, k + 5, -1, -1], [30, -1, -1, -1], [-1] * 4, [7, -1, -1, -1]]
    assert ok
    got = backing.cpu().numpy()
    for z in (0, 1, 2, 3, 4, 8, 9, 10, 11):
        assert np.array_equal(got[z, :, :S], good[z]), f"stripe {z}"
    assert (got[:, :, S:] == FILL).all()
    # stripes 5, 6, 7 were clean and are marked degraded: rebuilt to the codeword as well
    assert np.array_equal(got[:, :, :S], good)


def route_stats(reset=True):
    out = (C.c_uint64 * 3)()
    assert rs.lib().rs_debug_checked_stats(out, int(reset)) == 0
    return [int(x) for x in out]


@pytest.mark.parametrize("bits,k,p,S", [(16, 37, 9, 192), (8, 100, 28, 192)])
def test_passes_agree_and_rounds_are_bounded(bits, k, p, S, paths):
    """Passes of 1, of 5 and of the automatic size over the same slab: equal
    verdicts and bytes, and per pass at most cap confirm rounds and 1 + 2 cap
    host waits however many stripes it holds (rs_debug_checked_stats)."""
    good, bad, missing, corrupt = tamper(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    table = table_of(k, p, missing)
    want = expected(bits, k, p, missing, corrupt)
    nlist = sum(1 for z in range(NS) if z != 8 and want[z] != [])  # bad stripes with missing rows and cap_z >= 1
    nlist -= sum(1 for z in range(NS) if z != 8 and want[z] is None and cap_z(p, len(missing[z])) < 1)
    assert rs.lib().rs_debug_checked_stats(None, 0) != 0
    results = []
    for chunk in (1, 5, 0):
        paths("scrub_chunk", chunk)
        backing, slab = padded(prefill(bad, missing, 1))
        route_stats()
        count, shards = c.reconstruct_checked_dev_batch_patterns(slab, table, range(NS), repair=True)
        passes, rounds, waits = route_stats()
        assert passes == (1 if chunk == 0 else -(-nlist // chunk))
        assert rounds <= MAXS * passes and waits <= (1 + 2 * MAXS) * passes
        assert rounds >= 2, "stripe 3 (disjoint places) takes a second round wherever it sits"
        assert route_stats() == [0, 0, 0], "the read with reset clears the counters"
        results.append((count.tolist(), shards.tolist(), backing.cpu().numpy()))
    for r in results[1:]:
        assert r[0] == results[0][0] and r[1] == results[0][1] and np.array_equal(r[2], results[0][2])
    # a clean degraded slab never takes the route
    backing, slab = padded(prefill(good, missing, 0))
    c.reconstruct_checked_dev_batch_patterns(slab, table, range(NS))
    assert route_stats() == [0, 0, 0]
