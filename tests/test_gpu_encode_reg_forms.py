"""GPU tests of the register encode's three forms (kernels.hip encode_reg_body
behind k_encode_reg and k_encode_reg_list) against the oracle: rows by pointer
table, a strided batch with the stripe in grid.y, and a list of stripes of
different sizes.  One geometry per log2 m = 0..5 and field, p < m in three of
them (the `r < a.p` guards), k = 2m + 1 (three chunks, the last of one row).
After a call the whole buffer must be, bit for bit, the expected image: the
oracle's parity in the parity rows and every other byte (the gaps and the
padding behind each row) as it was.  Every comparison is exact.
"""
import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOMS = [(bits, 2 * (1 << lm) + 1, p) for bits in (8, 16) for lm, p in enumerate((1, 2, 3, 7, 13, 32))]
# 64: one unit, most lanes dead; 1088 / 4160 / 8256: one narrow GF(2^8), one
# wide GF(2^8), one wide GF(2^16) workgroup plus one unit (a dead wave joins the barriers)
SIZES = [64, 1088, 4160, 8256]
WIDTHS = [-1, 0, 1]
FILL = 0xA5
# the kernel a strided batch takes: the register kernel for GF(2^8) and GF(2^16) m <= 2
BATCH_PATH = {8: ["reg8-m1", "reg8-m2", "reg8-m4", "reg8-m8", "reg8-m16", "reg8-m32"],
              16: ["reg16-m1", "reg16-m2", "split16-m4", "split16-m8", "bs16-m16", "bs16-m32"]}

geoms = pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "gf%d-%d+%d" % g)
widths = pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "width%+d" % w)

_shards = {}


def shards(bits, k, p):
    """Per size the k data rows and the oracle's p parity rows as one (k+p, S)
    array: computed once per geometry, shared by the three forms, never written."""
    key = (bits, k, p)
    if key not in _shards:
        rng = np.random.default_rng(bits * 7919 + k * 131 + p * 17)
        out = []
        for S in SIZES:
            data = rng.integers(0, 256, (k, S), dtype=np.uint8)
            rows = np.concatenate([data, orc.encode(bits, k, p, data)])
            rows.setflags(write=False)
            out.append(rows)
        _shards[key] = out
    return _shards[key]


_second = {}


def second_stripe(bits, k, p, n):
    """Another stripe of size SIZES[n]: the first one's data rows in reverse order, encoded."""
    key = (bits, k, p, n)
    if key not in _second:
        data = np.ascontiguousarray(shards(bits, k, p)[n][:k][::-1])
        rows = np.concatenate([data, orc.encode(bits, k, p, data)])
        rows.setflags(write=False)
        _second[key] = rows
    return _second[key]


def images(nbytes, rows_at, k):
    """The buffer before a call (data rows in, FILL everywhere else, the parity
    rows included) and the expected image after it; rows_at: (offset, row) pairs
    of every stripe's rows, k data rows then the parity rows."""
    before = np.full(nbytes, FILL, np.uint8)
    want = before.copy()
    for off, i, row in rows_at:
        want[off: off + row.size] = row
        if i < k:
            before[off: off + row.size] = row
    return before, want


def flip(buf, at):
    buf[at] ^= 0x01


@geoms
@widths
def test_row_table(geom, width, paths):
    """Separately placed rows: in memory in another order than the stripe's,
    with gaps of different sizes between them, so no constant stride."""
    bits, k, p = geom
    paths("unit_width", width)
    c = rs.ReedSolomon(k, p, bits)
    for S, sh in zip(SIZES, shards(bits, k, p)):
        order = list(range(1, k + p, 2)) + list(range(0, k + p, 2))  # odd rows first
        off, at = [0] * (k + p), 128
        for n, i in enumerate(order):
            off[i] = at
            at += S + 64 * (1 + n % 3)
        before, want = images(at + 64, [(off[i], i, sh[i]) for i in range(k + p)], k)
        buf = torch.from_numpy(before).to(DEV)
        rows = [buf[o: o + S] for o in off]
        c.encode_dev(rows)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want), S
        assert c.verify_dev(rows) is True
        for pos in (off[k + p - 1] + S - 1, off[k - 1] + S - 1):  # last parity byte, last data row's last unit
            flip(buf, pos)
            assert c.verify_dev(rows) is False, (S, pos)
            flip(buf, pos)
        assert c.verify_dev(rows) is True
        assert np.array_equal(buf.cpu().numpy(), want), S  # verify wrote nothing
    c.close()


@geoms
@widths
def test_strided_batch(geom, width, paths):
    """Two stripes, row stride S + 64, a gap between the stripes."""
    bits, k, p = geom
    paths("unit_width", width)
    c = rs.ReedSolomon(k, p, bits)
    assert c.encode_path == BATCH_PATH[bits][(k - 1).bit_length() - 2]
    small = shards(bits, k, p)
    for n, S in enumerate(SIZES):
        st, base = S + 64, 192
        sstride = (k + p) * st + 320
        stripes = [small[n], second_stripe(bits, k, p, n)]
        rows_at = [(base + z * sstride + i * st, i, stripes[z][i]) for z in range(2) for i in range(k + p)]
        before, want = images(base + 2 * sstride, rows_at, k)
        buf = torch.from_numpy(before).to(DEV)
        slab = torch.as_strided(buf, (2, k + p, S), (sstride, st, 1), base)
        c.encode_dev_batch(slab)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want), S
        assert c.verify_dev_batch(slab) is True
        assert c.verify_dev_batch_map(slab).tolist() == [False, False]
        for z in range(2):
            for row in (k + p - 1, k - 1):  # last parity byte, last data row's last unit
                at = base + z * sstride + row * st + S - 1
                flip(buf, at)
                assert c.verify_dev_batch(slab) is False, (S, z, row)
                assert c.verify_dev_batch_map(slab).tolist() == [z == 0, z == 1], (S, z, row)
                flip(buf, at)
        assert c.verify_dev_batch_map(slab).tolist() == [False, False]
        assert np.array_equal(buf.cpu().numpy(), want), S  # verify wrote nothing
    c.close()


@geoms
@widths
def test_stripe_list(geom, width, paths):
    """The four sizes in one call, in memory in another order than the list's,
    with gaps, row strides S and S + 64."""
    bits, k, p = geom
    paths("unit_width", width)
    c = rs.ReedSolomon(k, p, bits)
    sh = shards(bits, k, p)
    where, at = [None] * len(SIZES), 64
    for z in (2, 0, 3, 1):
        st = SIZES[z] + 64 * (z % 2)
        where[z] = (at, st)
        at += (k + p - 1) * st + SIZES[z] + 64 * (1 + z)
    rows_at = [(off + i * st, i, sh[z][i]) for z, (off, st) in enumerate(where) for i in range(k + p)]
    before, want = images(at + 64, rows_at, k)
    buf = torch.from_numpy(before).to(DEV)
    stripes = [torch.as_strided(buf, (k + p, S), (st, 1), off) for S, (off, st) in zip(SIZES, where)]
    c.encode_dev_list(stripes)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)
    assert c.verify_dev_list(stripes).tolist() == [True] * len(SIZES)
    for z, (S, (off, st)) in enumerate(zip(SIZES, where)):
        for row in (k + p - 1, k - 1):  # last parity byte, last data row's last unit
            flip(buf, off + row * st + S - 1)
            assert c.verify_dev_list(stripes).tolist() == [y != z for y in range(len(SIZES))], (z, row)
            flip(buf, off + row * st + S - 1)
    assert c.verify_dev_list(stripes).tolist() == [True] * len(SIZES)
    assert np.array_equal(buf.cpu().numpy(), want)  # verify wrote nothing
    c.close()
