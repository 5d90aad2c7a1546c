"""GPU tests of the batched locate (rs_locate_dev_batch; stream_kernels.hip
k_syndrome_scan_list, k_syndrome_pick, k_syndrome_confirm, k_syndrome_fix) and
of rs_scrub_dev_batch routed through it, on oracle-encoded stripes in a padded
slab: every listed stripe gets rs_locate_dev's verdict, a located shard is
repaired bit for bit, and nothing else -- padding, clean stripes, corrupt
stripes that are not listed -- is written.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS, PAD, FILL = 12, 64, 0xA5
CLEAN, UNLOCATED = rs.SCRUB_CLEAN, rs.SCRUB_UNLOCATED
SKIPPED = 2  # a corrupt stripe the lists of test_repair_* leave out

# 4160 = three 2 KiB tiles per stripe, the last partial (the bit-sliced encode into the scratch rows)
ALL = (64, 192, 4160)
# (bits, k, p, sizes, path knobs): one geometry per verify path
GEOMS = [
    (16, 128, 32, ALL, {}),          # bit-sliced, m = 32
    (16, 37, 9, ALL, {}),            # bit-sliced, m = 16
    (16, 10, 4, ALL, {}),            # half-wave split
    (16, 3, 7, ALL, {}),             # k < m
    (16, 2, 1, ALL, {}),             # p = 1
    (16, 200, 100, (64, 192), {}),   # LDS, m = 128
    (8, 10, 4, ALL, {}),             # register, GF(2^8)
    (8, 128, 128, ALL, {}),          # LDS, GF(2^8)
    (16, 600, 300, (64,), {"lds_big": 0}),  # multi-pass
]
CASES = [pytest.param(b, k, p, S, knobs, id=f"{b}-{k}+{p}-S{S}") for b, k, p, sizes, knobs in GEOMS for S in sizes]

_slabs = {}


def stripes(bits, k, p, S, n=NS):
    """n oracle-encoded stripes [n, k+p, S] for a geometry and size, computed once and never written."""
    key = (bits, k, p, S, n)
    if key not in _slabs:
        rng = np.random.default_rng(bits * 7919 + k * 131 + p * 17 + S + n)
        out = np.empty((n, k + p, S), np.uint8)
        for z in range(n):
            out[z, :k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
            out[z, k:] = orc.encode(bits, k, p, out[z, :k])
        out.setflags(write=False)
        _slabs[key] = out
    return _slabs[key]


def padded(content):
    """content [n, rows, S] inside a padded backing tensor: (backing, the strided view of the content)."""
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


def tamper(good, bits, k, p):
    """A copy of `good` with, by stripe: 0 a bit of the first byte of a data
    row; 1 a bit of the last byte of the last data row; 2 a data row replaced;
    3 parity row 0; 4 parity row 1; 5 a parity row >= 2 (the last one where
    there are fewer); 6 a bit in a GF(2^16) high-byte half; 7 two data shards
    at different symbols (the ratio at the first names shard 0, only the
    confirm refutes it); 8 a data shard and a parity shard; 9 stripe 0's data
    shard again (a shared column table); 10 and 11 clean.  Returns (bad slab,
    expected verdicts)."""
    S = good.shape[2]
    rng = np.random.default_rng(k * 977 + p * 31 + S)
    bad = np.array(good)
    j0, j2, j6, j8 = (int(rng.integers(0, k)) for _ in range(4))
    bad[0, j0, 0] ^= 0x10
    bad[1, k - 1, S - 1] ^= 0x01
    row = rng.integers(0, 256, S, dtype=np.uint8)
    row[7] = good[2, j2, 7] ^ 0x80  # (certainly another row)
    bad[2, j2] = row
    bad[3, k, S // 2] ^= 0x04
    p1 = min(p - 1, 1)
    bad[4, k + p1, S - 1] ^= 0x80
    pi = min(p - 1, 2 + int(rng.integers(0, max(p - 2, 1))))
    bad[5, k + pi, 1] ^= 0x40
    bad[6, j6, S - 64 + 32 + 5] ^= 0x08
    bad[7, 0, 3] ^= 0x20
    bad[7, 1, S - 5] ^= 0x02
    bad[8, j8, 9] ^= 0x11
    bad[8, k + p - 1, 9] ^= 0x01
    bad[9, j0, S - 2] ^= 0xFF
    if p == 1:
        want = [UNLOCATED] * 10 + [CLEAN] * 2
    else:
        want = [j0, k - 1, j2, k, k + p1, k + pi, j6, UNLOCATED, UNLOCATED, j0, CLEAN, CLEAN]
    return bad, np.array(want, np.int32)


def scrub(c, slab, repair):
    """rs_scrub_dev_batch with its nbad."""
    n, _, S = slab.shape
    verdict = np.full(n, 77, np.int32)
    nbad = C.c_int(-1)
    e = c._L.rs_scrub_dev_batch(c._h, slab.data_ptr(), slab.stride(1), slab.stride(0), n, S, int(repair),
                                verdict.ctypes.data, C.byref(nbad), None)
    assert e == 0, e
    return verdict, nbad.value


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_verdicts_equal_locate_dev(bits, k, p, S, knobs, paths):
    good = stripes(bits, k, p, S)
    bad, want = tamper(good, bits, k, p)
    c = codec(bits, k, p, knobs, paths)
    backing, slab = padded(bad)
    before = backing.clone()
    v = c.locate_dev_batch(slab, range(NS))
    assert v.dtype == np.int32 and v.tolist() == want.tolist()
    assert torch.equal(backing, before), "repair=0 wrote something"
    copy = before.clone()[:, :, :S]
    one = [c.locate_dev([copy[z, i] for i in range(k + p)]) for z in range(NS)]
    assert v.tolist() == one, "rs_locate_dev, stripe by stripe, says otherwise"
    # a list of clean stripes only, and an empty one
    assert c.locate_dev_batch(slab, [11, 10]).tolist() == [CLEAN, CLEAN]
    assert c.locate_dev_batch(slab, []).tolist() == []
    assert torch.equal(backing, before)


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_repair_shuffled_list_in_chunks(bits, k, p, S, knobs, paths):
    """A shuffled list without stripe SKIPPED, in passes of 1, of 5 (two and a
    remainder of one) and of the automatic size: the permuted verdicts, the
    located shards restored, the unlisted corrupt stripe as it was."""
    good = stripes(bits, k, p, S)
    bad, want = tamper(good, bits, k, p)
    c = codec(bits, k, p, knobs, paths)
    rng = np.random.default_rng(S + k)
    lst = [int(z) for z in rng.permutation(NS) if z != SKIPPED]
    results = []
    for chunk in (1, 5, 0):
        paths("scrub_chunk", chunk)
        backing, slab = padded(bad)
        v = c.locate_dev_batch(slab, lst, repair=True)
        assert v.tolist() == [int(want[z]) for z in lst], f"chunk {chunk}"
        got = backing.cpu().numpy()
        assert (got[:, :, S:] == FILL).all(), "padding bytes written"
        for z in range(NS):
            fixed = z != SKIPPED and want[z] >= 0
            assert np.array_equal(got[z, :, :S], good[z] if fixed else bad[z]), f"chunk {chunk} stripe {z}"
        again = c.locate_dev_batch(slab, lst, repair=True)
        assert again.tolist() == [UNLOCATED if want[z] == UNLOCATED else CLEAN for z in lst]
        assert np.array_equal(backing.cpu().numpy(), got), "the second call wrote something"
        results.append(got)
    assert all(np.array_equal(results[0], r) for r in results[1:])


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_scrub_routes_agree(bits, k, p, S, knobs, paths):
    """rs_scrub_dev_batch one stripe at a time ("scrub_batch" 0) and through the
    batched locate (1): equal verdicts, equal nbad, equal slabs."""
    good = stripes(bits, k, p, S)
    bad, want = tamper(good, bits, k, p)
    c = codec(bits, k, p, knobs, paths)
    out = {}
    for route in (0, 1):
        paths("scrub_batch", route)
        backing, slab = padded(bad)
        before = backing.clone()
        v0, n0 = scrub(c, slab, 0)
        assert torch.equal(backing, before), f"route {route}: repair=0 wrote something"
        v1, n1 = scrub(c, slab, 1)
        out[route] = (v0.tolist(), n0, v1.tolist(), n1, backing.cpu().numpy())
    assert out[0][:4] == out[1][:4]
    assert np.array_equal(out[0][4], out[1][4])
    assert out[1][0] == want.tolist() and out[1][1] == 10
    got = out[1][4]
    for z in range(NS):
        assert np.array_equal(got[z, :, :S], good[z] if want[z] >= 0 else bad[z]), f"stripe {z}"
    assert (got[:, :, S:] == FILL).all(), "padding bytes written"


@pytest.mark.parametrize("null_stream", [False, True])
def test_locate_batch_is_stream_ordered(null_stream, paths):
    """The corruption is a torch op on the stream and the call is queued right
    behind it: no synchronise in between."""
    bits, k, p, S = 16, 37, 9, 4160
    good = stripes(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    paths("scrub_chunk", 2)
    backing, slab = padded(good)
    mask = torch.zeros(S, dtype=torch.uint8, device=DEV)
    mask[100:164] = 0x5A
    torch.cuda.synchronize()
    st = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    with torch.cuda.stream(st):
        slab[2, 11] ^= mask
        slab[3, k + 4] ^= mask
        slab[7, 36] ^= mask
        v = c.locate_dev_batch(slab, [7, 0, 3, 2, 11], repair=True, stream=st)
        ok = c.verify_dev_batch(slab, stream=st)
    assert v.tolist() == [36, CLEAN, k + 4, 11, CLEAN]
    assert ok
    assert np.array_equal(slab.cpu().numpy(), good)
    assert bool((backing[:, :, S:] == FILL).all())


def test_candidates_of_more_columns_than_one_column_set():
    """12+32768: a column's tables take 3 MiB, so the 32 MiB table bound holds 8
    columns; candidates in ten distinct columns are confirmed in two passes
    (8 + 2).  Ten copies of one stripe, stripe z bad in data shard z, an
    eleventh bad in two shards, a twelfth clean."""
    bits, k, p, S, n = 16, 12, 32768, 64, 12
    rng = np.random.default_rng(12 + 32768)
    one = np.empty((k + p, S), np.uint8)
    one[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
    one[k:] = orc.encode(bits, k, p, one[:k])
    good = np.repeat(one[None], n, axis=0)
    bad = good.copy()
    for z in range(10):
        bad[z, z, 5 * z] ^= 0x21
    bad[10, 3, 0] ^= 1
    bad[10, 11, 40] ^= 1
    want = list(range(10)) + [UNLOCATED, CLEAN]
    c = rs.ReedSolomon(k, p, bits)
    backing, slab = padded(bad)
    assert c.locate_dev_batch(slab, range(n)).tolist() == want
    assert c.locate_dev_batch(slab, range(n), repair=True).tolist() == want
    got = backing.cpu().numpy()
    assert np.array_equal(got[:10, :, :S], good[:10]) and np.array_equal(got[10:, :, :S], bad[10:])
    assert (got[:, :, S:] == FILL).all()


def test_three_hundred_bad_stripes():
    """Every stripe bad in data shard z mod 10: ten column tables shared by 300
    candidates of one pass, all located and repaired."""
    bits, k, p, S, n = 16, 10, 4, 64, 300
    good = stripes(bits, k, p, S, n)
    bad = np.array(good)
    for z in range(n):
        bad[z, z % k, (7 * z) % S] ^= 1 + z % 255
    c = rs.ReedSolomon(k, p, bits)
    backing, slab = padded(bad)
    v = c.locate_dev_batch(slab, range(n), repair=True)
    assert v.tolist() == [z % k for z in range(n)]
    got = backing.cpu().numpy()
    assert np.array_equal(got[:, :, :S], good)
    assert (got[:, :, S:] == FILL).all()
    assert (c.locate_dev_batch(slab, range(n)) == CLEAN).all()
