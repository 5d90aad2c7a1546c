"""GPU tests of the encode and verify of a list of stripes of different sizes
(rs_encode_dev_list / rs_verify_dev_list; kernels.hip k_encode_reg_list)
against the oracle: after a call the whole buffer that holds the stripes must
be, bit for bit, the expected image -- the oracle's parity in every stripe's p
parity rows and every other byte as it was.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc
from reedsolomon16_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIST_GEOMS = [(8, 10, 4), (8, 100, 28), (16, 2, 1), (16, 3, 7), (16, 37, 9), (16, 128, 32)]  # through the list kernel
LOOP_GEOMS = [(8, 128, 128), (16, 300, 300)]                                                  # through the fallback loop
GEOMS = LIST_GEOMS + LOOP_GEOMS
# The workgroup spans of the narrow and wide units of both fields, and each
# plus one unit: 64 is one unit with most lanes dead; 1024 / 4096 one narrow /
# wide GF(2^8) workgroup; 8192 one wide GF(2^16) workgroup.
SIZES = [64, 192, 1024, 1088, 4096, 4160, 8192, 8256, 64]
PLACE = [4, 0, 7, 2, 8, 5, 1, 6, 3]  # the stripes' order in memory: not the list's
# (enc_list, unit_width): every routing at the automatic width, both widths at the automatic routing
KNOBS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (-1, 1)]


def NS():
    """The C-ABI handle of torch's current stream: the calls stay ordered with torch's own work."""
    return rs.codec._stream_handle(None)


def row_stride(z, S):
    return (S, S + 64, 2 * S)[z % 3]


_cases = {}


def case(bits, k, p):
    """Per stripe (offset, row stride, size), the buffer before the call (data
    in, 0xA5 everywhere else, the parity rows included) and the expected image
    after it: computed once per geometry, shared by the tests, never written."""
    key = (bits, k, p)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(bits * 7919 + k * 131 + p * 17)
    where, at = [None] * len(SIZES), 64
    for z in PLACE:
        S = SIZES[z]
        st = row_stride(z, S)
        where[z] = (at, st, S)
        at += (k + p - 1) * st + S + 64 * (1 + z % 3)  # a gap after every stripe
    before = np.full(at + 64, 0xA5, np.uint8)
    want = before.copy()
    for z, (off, st, S) in enumerate(where):
        data = rng.integers(0, 256, (k, S), dtype=np.uint8)
        par = orc.encode(bits, k, p, data)
        for i in range(k + p):
            row = data[i] if i < k else par[i - k]
            want[off + i * st: off + i * st + S] = row
            if i < k:
                before[off + i * st: off + i * st + S] = row
    before.setflags(write=False)
    want.setflags(write=False)
    _cases[key] = (where, before, want)
    return _cases[key]


def views(buf, where, k, p):
    return [torch.as_strided(buf, (k + p, S), (st, 1), off) for off, st, S in where]


def test_layout():
    """The list has the shape the other tests are meant to cover."""
    where, before, _ = case(8, 10, 4)
    offs = [w[0] for w in where]
    assert offs != sorted(offs)
    assert {w[1] - w[2] for w in where} >= {0, 64} and any(w[1] == 2 * w[2] for w in where)
    spans = sorted((off, off + 13 * st + S) for off, st, S in where)
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))  # disjoint, with gaps
    assert spans[0][0] > 0 and spans[-1][1] < before.size


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda kn: "list%+d-width%+d" % kn)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "gf%d-%d+%d" % g)
def test_encode_and_verify(geom, knobs, paths):
    bits, k, p = geom
    where, before, want = case(bits, k, p)
    paths("enc_list", knobs[0])
    paths("unit_width", knobs[1])
    c = rs.ReedSolomon(k, p, bits)
    buf = torch.from_numpy(np.array(before)).to(DEV)
    stripes = views(buf, where, k, p)
    c.encode_dev_list(stripes)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)

    # verify: the clean list
    assert c.verify_dev_list(stripes).tolist() == [True] * len(SIZES)
    # one parity byte of stripe 2, one data byte in the last unit of stripe 7, and
    # the last byte of the largest stripe's last parity row (stripe 7 as well)
    assert max(range(len(SIZES)), key=lambda z: SIZES[z]) == 7
    stripes[2][k + p // 2, 77] ^= 0x10
    stripes[7][k - 1, SIZES[7] - 3] ^= 0x01
    stripes[7][k + p - 1, SIZES[7] - 1] ^= 0x80
    v = np.full(len(SIZES), 7, np.int8)
    ok = C.c_int(7)
    arr = c._stripe_list(stripes)
    assert c._L.rs_verify_dev_list(c._h, arr, len(stripes), v.ctypes.data, C.byref(ok), NS()) == 0
    assert v.tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1] and ok.value == 0
    # each of stripe 7's flips alone
    stripes[2][k + p // 2, 77] ^= 0x10
    stripes[7][k - 1, SIZES[7] - 3] ^= 0x01
    assert c.verify_dev_list(stripes).tolist() == [z != 7 for z in range(len(SIZES))]
    stripes[7][k + p - 1, SIZES[7] - 1] ^= 0x80
    stripes[7][k - 1, SIZES[7] - 3] ^= 0x01
    assert c.verify_dev_list(stripes).tolist() == [z != 7 for z in range(len(SIZES))]
    stripes[7][k - 1, SIZES[7] - 3] ^= 0x01
    assert c._L.rs_verify_dev_list(c._h, arr, len(stripes), None, C.byref(ok), NS()) == 0 and ok.value == 1
    # verify wrote nothing
    assert np.array_equal(buf.cpu().numpy(), want)
    c.close()


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "gf%d-%d+%d" % g)
def test_equals_batch_encode(geom):
    """On a uniform slab the list call writes what rs_encode_dev_batch writes, stripe by stripe."""
    bits, k, p = geom
    rng = np.random.default_rng(k + p)
    c = rs.ReedSolomon(k, p, bits)
    for S in (192, 4160):
        slab = torch.from_numpy(rng.integers(0, 256, (3, k + p, S), dtype=np.uint8)).to(DEV)
        ref = slab.clone()
        c.encode_dev_list([slab[z] for z in range(3)])
        for z in range(3):
            c._L.rs_encode_dev_batch(c._h, ref[z].data_ptr(), S, 0, 1, S, rs.codec._stream_handle(None))
        torch.cuda.synchronize()
        assert torch.equal(slab, ref)
    c.close()


def test_many_stripes():
    """200 000 stripes of 2+1 x 64 bytes with one 8256-byte stripe in the middle:
    crosses a ring-slot cut and searches a long prefix.  16 distinct small
    stripes, tiled, so the oracle runs 17 times."""
    bits, k, p, n, S, BIG = 16, 2, 1, 200_000, 64, 8256
    rng = np.random.default_rng(99)
    tile = rng.integers(0, 256, (16, k + p, S), dtype=np.uint8)
    tile_want = tile.copy()
    for t in range(16):
        tile_want[t, k:] = orc.encode(bits, k, p, tile[t, :k])
    big = rng.integers(0, 256, (k + p, BIG), dtype=np.uint8)
    big_want = big.copy()
    big_want[k:] = orc.encode(bits, k, p, big[:k])
    half, small = n // 2, (k + p) * S

    def image(t, b):
        return np.concatenate([np.tile(t, (half // 16, 1, 1)).ravel(), b.ravel(), np.tile(t, (half // 16, 1, 1)).ravel(),
                               np.full(256, 0xA5, np.uint8)])

    buf = torch.from_numpy(image(tile, big)).to(DEV)
    want = torch.from_numpy(image(tile_want, big_want)).to(DEV)
    base = buf.data_ptr()
    # the list, straight as rs_stripe records: the first half, the big stripe, the second half
    rec = np.zeros(n + 1, dtype=[("base", "<u8"), ("stride", "<u8"), ("size", "<u8")])
    z = np.arange(n + 1, dtype=np.uint64)
    rec["base"] = base + np.where(z <= half, z * small, (z - 1) * small + (k + p) * BIG)
    rec["stride"], rec["size"] = S, S
    rec["stride"][half], rec["size"][half] = BIG, BIG
    arr = (_capi.Stripe * (n + 1)).from_buffer(rec)
    c = rs.ReedSolomon(k, p, bits)
    assert c._L.rs_encode_dev_list(c._h, arr, n + 1, NS()) == 0
    assert torch.equal(buf, want)
    v = np.full(n + 1, 7, np.int8)
    ok = C.c_int(7)
    assert c._L.rs_verify_dev_list(c._h, arr, n + 1, v.ctypes.data, C.byref(ok), NS()) == 0
    assert ok.value == 1 and v.all() and v.max() == 1
    bad = [3, half - 1, half, half + 1, 150_000, n]
    for b in bad:
        off = int(rec["base"][b]) - base
        buf[off + 5] ^= 1
    assert c._L.rs_verify_dev_list(c._h, arr, n + 1, v.ctypes.data, C.byref(ok), NS()) == 0
    assert ok.value == 0 and np.flatnonzero(v == 0).tolist() == bad and set(v.tolist()) == {0, 1}
    c.close()


@pytest.mark.parametrize("null_stream", [False, True], ids=["side-stream", "null-stream"])
@pytest.mark.parametrize("geom", [(8, 10, 4), (16, 128, 32), (8, 128, 128)], ids=lambda g: "gf%d-%d+%d" % g)
def test_stream_order(geom, null_stream):
    """The call is ordered on its stream: the data it reads is made by the
    kernel before it and its parity is read by the kernel after it, with no
    host wait between."""
    bits, k, p = geom
    where, before, want = case(bits, k, p)
    c = rs.ReedSolomon(k, p, bits)
    masked = torch.from_numpy(before ^ 0x5A).to(DEV)
    buf = torch.empty_like(masked)
    stripes = views(buf, where, k, p)
    torch.cuda.synchronize()
    st = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    if null_stream:
        assert rs.codec._stream_handle(st) == rs.codec.RS_NULL_STREAM
    with torch.cuda.stream(st):
        torch.bitwise_xor(masked, 0x5A, out=buf)
        c.encode_dev_list(stripes, stream=st)
        got = buf.clone()
    st.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    c.close()


def test_stripes_split_between_the_list_and_their_own_kernel():
    """One call whose stripes part ways: at 128+32 (bit-sliced, m = 32) a stripe
    64 bytes above the 256 KiB threshold takes a launch of its own kernel, the
    small stripes before and after it share the list launch.  The parity of all
    of them, and the verdicts, which the call keeps in another order than the
    list's (list stripes first), must come back under the right stripe."""
    bits, k, p = 16, 128, 32
    sizes = [192, (256 << 10) + 64, 4160, 64]
    rng = np.random.default_rng(4242)
    where, at = [None] * len(sizes), 128
    for z in (2, 1, 3, 0):  # the order in memory
        where[z] = (at, sizes[z] + 64, sizes[z])
        at += (k + p) * (sizes[z] + 64) + 64
    before = np.full(at, 0xA5, np.uint8)
    want = before.copy()
    for off, st, S in where:
        data = rng.integers(0, 256, (k, S), dtype=np.uint8)
        par = orc.encode(bits, k, p, data)
        for i in range(k + p):
            want[off + i * st: off + i * st + S] = data[i] if i < k else par[i - k]
            if i < k:
                before[off + i * st: off + i * st + S] = data[i]
    c = rs.ReedSolomon(k, p, bits)
    assert c.encode_path == "bs16-m32"
    assert [c._L.rs_debug_encode_list_own(c._h, S) for S in sizes] == [0, 1, 0, 0]
    buf = torch.from_numpy(before).to(DEV)
    stripes = views(buf, where, k, p)
    c.encode_dev_list(stripes)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)
    assert c.verify_dev_list(stripes).tolist() == [True] * 4
    for bad in ([2], [1], [0, 1], [3]):
        for z in bad:
            stripes[z][k + 5 if z != 1 else 7, sizes[z] - 2] ^= 0x40  # the big stripe: a data byte
        assert c.verify_dev_list(stripes).tolist() == [z not in bad for z in range(4)]
        for z in bad:
            stripes[z][k + 5 if z != 1 else 7, sizes[z] - 2] ^= 0x40
    assert np.array_equal(buf.cpu().numpy(), want)
    # the mirror takes uint8 tensors on the codec's device only
    with pytest.raises(TypeError):
        c.encode_dev_list([s.view(torch.int8) for s in stripes])
    c.close()
