"""GPU tests of the scrub (rs_verify_dev_batch_map, rs_locate_dev,
rs_scrub_dev_batch; stream_kernels.hip k_syndrome_scan and the per-stripe mismatch
words of the verify kernels) on oracle-encoded stripes: a tampered shard must
be named, repaired bit for bit, and nothing else written.
"""
import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS, PAD, FILL = 5, 64, 0xA5
CLEAN, UNLOCATED = rs.SCRUB_CLEAN, rs.SCRUB_UNLOCATED

# 4160 = three 2 KiB tiles per stripe, the last partial: the bit-sliced kernel's
# tile -> stripe division has a remainder
ALL = (64, 192, 4160)
# (bits, k, p, sizes, path knobs): one geometry per verify path
GEOMS = [
    (16, 128, 32, ALL, {}),          # bit-sliced, m = 32
    (16, 37, 9, ALL, {}),            # bit-sliced, m = 16
    (16, 20, 12, ALL, {}),           # bit-sliced, m = 16
    (16, 10, 4, ALL, {}),            # half-wave split
    (16, 3, 7, ALL, {}),             # k < m
    (16, 2, 1, ALL, {}),             # p = 1
    (16, 1, 1, ALL, {}),             # p = 1
    (16, 200, 100, (64, 192), {}),   # LDS, m = 128
    (16, 1024, 256, (64, 192), {}),  # LDS, m = 256
    (8, 10, 4, ALL, {}),             # register, GF(2^8)
    (8, 100, 28, ALL, {}),           # register, GF(2^8), m = 32
    (8, 128, 128, ALL, {}),          # LDS, GF(2^8)
    (16, 600, 300, (64,), {"lds_big": 0}),  # multi-pass
]
CASES = [pytest.param(b, k, p, S, knobs, id=f"{b}-{k}+{p}-S{S}") for b, k, p, sizes, knobs in GEOMS for S in sizes]

_slabs = {}


def stripes(bits, k, p, S):
    """NS oracle-encoded stripes [NS, k+p, S] for a geometry and size, computed once and never written."""
    key = (bits, k, p, S)
    if key not in _slabs:
        rng = np.random.default_rng(bits * 7919 + k * 131 + p * 17 + S)
        out = np.empty((NS, k + p, S), np.uint8)
        for z in range(NS):
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
    """A copy of `good` with stripe 0: one bit of the first byte of a data row
    flipped; 1: one bit of the last byte of the last data row; 2: a data row
    replaced by random bytes; 3: a parity row >= 2 (where there is one)
    tampered; 4: two shards tampered.  Returns (bad slab, expected verdicts)."""
    S = good.shape[2]
    rng = np.random.default_rng(k * 977 + p * 31 + S)
    bad = np.array(good)
    j0, j2 = int(rng.integers(0, k)), int(rng.integers(0, k))
    bad[0, j0, 0] ^= 0x10
    bad[1, k - 1, S - 1] ^= 0x01
    row = rng.integers(0, 256, S, dtype=np.uint8)
    row[7] = good[2, j2, 7] ^ 0x80  # (certainly another row)
    bad[2, j2] = row
    pi = min(p - 1, 2 + int(rng.integers(0, max(p - 2, 1))))
    bad[3, k + pi, S // 2] ^= 0x04
    bad[4, 0, 3] ^= 0x20
    bad[4, k if k == 1 else 1, S - 5] ^= 0x02
    want = [j0, k - 1, j2, k + pi, UNLOCATED] if p > 1 else [UNLOCATED] * NS
    return bad, np.array(want, np.int32)


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_clean_batch_and_map(bits, k, p, S, knobs, paths):
    good = stripes(bits, k, p, S)
    c = codec(bits, k, p, knobs, paths)
    backing, slab = padded(good)
    before = backing.clone()
    assert not c.verify_dev_batch_map(slab).any()
    v = c.scrub_dev_batch(slab, repair=True)
    assert v.dtype == np.int32 and (v == CLEAN).all()
    assert c.verify_dev_batch(slab)
    assert torch.equal(backing, before), "a clean scrub wrote something"
    # stripes 0 and 4 bad, 1-3 clean: a data byte and a parity byte
    bad = np.array(good)
    bad[0, k // 2, S - 1] ^= 0x40
    bad[4, k + p - 1, 0] ^= 0x01
    backing, slab = padded(bad)
    before = backing.clone()
    got = c.verify_dev_batch_map(slab)
    assert got.dtype == bool and got.tolist() == [True, False, False, False, True]
    assert not c.verify_dev_batch(slab), "the existing call keeps its result"
    assert c.verify_dev_batch(slab[1:4])
    assert torch.equal(backing, before), "the map wrote something"


@pytest.mark.parametrize("bits,k,p,S,knobs", CASES)
def test_scrub_locates_and_repairs(bits, k, p, S, knobs, paths):
    good = stripes(bits, k, p, S)
    bad, want = tamper(good, bits, k, p)
    c = codec(bits, k, p, knobs, paths)
    backing, slab = padded(bad)
    before = backing.clone()
    v = c.scrub_dev_batch(slab, repair=False)
    assert v.tolist() == want.tolist()
    assert torch.equal(backing, before), "repair=0 wrote something"
    assert c.verify_dev_batch_map(slab).all()
    v = c.scrub_dev_batch(slab, repair=True)
    assert v.tolist() == want.tolist()
    got = backing.cpu().numpy()
    assert (got[:, :, S:] == FILL).all(), "padding bytes written"
    for z in range(NS):
        fixed = want[z] >= 0
        assert np.array_equal(got[z, :, :S], good[z] if fixed else bad[z]), f"stripe {z}"
    again = c.scrub_dev_batch(slab, repair=True)
    assert again.tolist() == [CLEAN if w >= 0 else UNLOCATED for w in want]
    assert np.array_equal(backing.cpu().numpy(), got), "the second scrub wrote something"


@pytest.mark.parametrize("bits,k,p", [(16, 128, 32), (16, 10, 4), (16, 200, 100), (8, 100, 28), (16, 2, 1)])
def test_locate_dev_scattered_rows(bits, k, p):
    """Row pointers of separate allocations; the flipped bit sits in the
    high-byte half of a GF(2^16) block."""
    S = 192
    good = stripes(bits, k, p, S)[1]
    c = rs.ReedSolomon(k, p, bits)
    rows = [torch.from_numpy(np.array(good[i])).to(DEV) for i in range(k + p)]
    assert c.locate_dev(rows) == CLEAN
    j = k - 1
    rows[j][64 + 32 + 5] ^= 0x08
    want = j if p > 1 else UNLOCATED
    assert c.locate_dev(rows) == want
    assert rows[j].cpu().numpy()[64 + 32 + 5] == good[j, 64 + 32 + 5] ^ 0x08, "repair=0 wrote the row"
    assert c.locate_dev(rows, repair=True) == want
    if p == 1:
        return
    for i in range(k + p):
        assert np.array_equal(rows[i].cpu().numpy(), good[i]), f"row {i}"
    assert c.locate_dev(rows) == CLEAN
    rows[k + 1][0] ^= 0xFF  # a parity row
    assert c.locate_dev(rows, repair=True) == k + 1
    for i in range(k + p):
        assert np.array_equal(rows[i].cpu().numpy(), good[i]), f"row {i}"
    # a 2-D tensor works as the row set too
    t = torch.from_numpy(np.array(good)).to(DEV)
    t[0, S - 1] ^= 1
    assert c.locate_dev(t, repair=True) == 0
    assert np.array_equal(t.cpu().numpy(), good)


@pytest.mark.parametrize("null_stream", [False, True])
def test_scrub_is_stream_ordered(null_stream):
    """The corruption is a torch op on the stream and the scrub is queued right
    behind it: no synchronise in between."""
    bits, k, p, S = 16, 37, 9, 4160
    good = stripes(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    backing, slab = padded(good)
    mask = torch.zeros(S, dtype=torch.uint8, device=DEV)
    mask[100:164] = 0x5A
    torch.cuda.synchronize()
    st = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    with torch.cuda.stream(st):
        slab[2, 11] ^= mask
        slab[3, k + 4] ^= mask
        v = c.scrub_dev_batch(slab, repair=True, stream=st)
        ok = c.verify_dev_batch(slab, stream=st)
    assert v.tolist() == [CLEAN, CLEAN, 11, k + 4, CLEAN]
    assert ok
    assert np.array_equal(slab.cpu().numpy(), good)


def test_many_stripes_cross_the_grid_slice():
    """32 770 copies of one 40+40 stripe (LDS encode): stripes on both sides of
    the 32 768-stripe grid slice are tampered, each in another shard."""
    bits, k, p, S, n = 16, 40, 40, 64, 32770
    one = stripes(bits, k, p, S)[0]
    c = rs.ReedSolomon(k, p, bits)
    ref = torch.from_numpy(np.array(one)).to(DEV)
    slab = ref.unsqueeze(0).repeat(n, 1, 1)
    hits = {0: 3, 32767: k + 7, 32768: 39, 32769: 0}
    for z, s in hits.items():
        slab[z, s, 9] ^= 0x81
    got = c.verify_dev_batch_map(slab)
    assert np.flatnonzero(got).tolist() == sorted(hits)
    v = c.scrub_dev_batch(slab, repair=True)
    assert np.flatnonzero(v != CLEAN).tolist() == sorted(hits)
    assert [int(v[z]) for z in sorted(hits)] == [hits[z] for z in sorted(hits)]
    assert bool((slab == ref.unsqueeze(0)).all()), "repair did not restore the slab"
    assert not c.verify_dev_batch_map(slab).any()
