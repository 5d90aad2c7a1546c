"""CPU tests of rs_locate_dev_batch's host side: its error rules, which are all
decided before any device call, the two path knobs of the batched scrub, and
the identity its confirm kernel checks in place of a full verify, against the
oracle: with one corrupt data row j the syndrome rows satisfy
e_i == G[i][j] * scale * e_0 for every parity row i, and with two corrupt data
rows some row violates it.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from oracle import leopard_np, orc
from reedsolomon16_amd import _capi

# test_scrub_cpu.py's ten geometries
GEOMS16 = [(128, 32), (37, 9), (3, 7), (2, 1), (1, 1), (1024, 256), (5, 2)]
GEOMS8 = [(10, 4), (100, 28), (128, 128)]
GEOMS = [(16, k, p) for k, p in GEOMS16] + [(8, k, p) for k, p in GEOMS8]

FAKE = 0x10000  # a non-NULL "device pointer": every call below must return before it is used
OK, INV, NO_DATA, BAD_SIZE, PANIC = 0, 53, 4, 6, 50


def u32(vals):
    return (C.c_uint32 * max(len(vals), 1))(*vals)


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(4, 2)
    multi = rs.New16(4, 2, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def test_locate_dev_batch_errors(codecs):
    one, multi = codecs
    L, h, S = _capi.lib(), one._h, 128
    verdict = (C.c_int32 * 4)(7, 7, 7, 7)
    BIG = 1 << 31  # INT32_MAX + 1

    def call(c=h, base=FAKE, rs_=S, ss=6 * S, ns=4, zs=(2, 0), nl=None, size=S, repair=0, v=verdict, nozs=False):
        arr = None if nozs else u32(zs)
        return L.rs_locate_dev_batch(c, base, rs_, ss, ns, arr, len(zs) if nl is None else nl, size, repair, v, None)

    # RS_ERR_INVALID_ARG: arguments, counts, the codec, the list
    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(nozs=True) == INV
    assert call(v=None) == INV
    assert call(nozs=True, nl=0) == INV      # NULL stripes even for an empty list
    assert call(v=None, nl=0) == INV
    assert call(ns=BIG) == INV
    assert call(nl=BIG) == INV
    assert call(c=multi._h) == INV           # a valid list on a multi-device codec
    assert call(c=multi._h, repair=1) == INV
    assert call(zs=(0, 4)) == INV            # stripes[e] >= nstripes
    assert call(zs=(3,), ns=3) == INV
    assert call(zs=(0,), ns=0) == INV
    assert call(zs=(1, 2, 1)) == INV         # the same stripe twice
    assert call(zs=(3, 3), repair=1) == INV
    # ... all before the size rules
    assert call(zs=(1, 1), size=0) == INV
    assert call(zs=(9,), size=100) == INV
    assert call(c=multi._h, size=0) == INV
    assert call(v=None, size=0, rs_=0) == INV
    # the size rules, then the stride rule
    assert call(size=0) == NO_DATA
    assert call(size=0, rs_=0) == NO_DATA
    assert call(size=100) == BAD_SIZE
    assert call(size=100, rs_=64) == BAD_SIZE
    assert call(size=192, rs_=128) == INV    # row_stride < shard_size
    assert call(size=0, zs=(), ns=0) == NO_DATA  # ... and before the empty list
    assert call(size=192, rs_=128, zs=()) == INV
    # an empty list is served without a device call
    assert call(zs=()) == OK
    assert call(zs=(), ns=0) == OK
    assert call(zs=(), repair=1) == OK
    assert list(verdict) == [7, 7, 7, 7], "an error or an empty list wrote a verdict"


def test_panic_geometry_is_refused_before_any_device_call():
    """GF(2^8) 250+6: the reference's encode panics, so there is no parity to recompute."""
    c = rs.New8(250, 6)
    L, S = _capi.lib(), 64
    verdict = (C.c_int32 * 2)()
    assert L.rs_locate_dev_batch(c._h, FAKE, S, 256 * S, 2, u32([1, 0]), 2, S, 1, verdict, None) == PANIC
    assert L.rs_locate_dev_batch(c._h, FAKE, S, 256 * S, 2, u32([]), 0, S, 0, verdict, None) == PANIC  # before nlist == 0
    assert L.rs_locate_dev_batch(c._h, FAKE, S, 256 * S, 2, u32([1, 1]), 2, S, 0, verdict, None) == INV
    assert L.rs_locate_dev_batch(c._h, FAKE, 32, 256 * S, 2, u32([1]), 1, S, 0, verdict, None) == INV  # the stride rule first
    c.close()


def test_knobs():
    L = _capi.lib()
    try:
        for v in (-1, 0, 1):
            _capi.set_path("scrub_batch", v)
        for v in (-2, 2, 100):
            assert L.rs_debug_set_path(b"scrub_batch", v) == INV
        for v in (0, 1, 5, 32768, 1 << 20):
            _capi.set_path("scrub_chunk", v)
        assert L.rs_debug_set_path(b"scrub_chunk", -1) == INV
        with pytest.raises(ValueError):
            _capi.set_path("scrub_chunk", -3)
        assert L.rs_debug_set_path(b"scrub_chunks", 1) == INV
    finally:
        _capi.reset_paths()
    assert _capi._PATH_DEFAULTS["scrub_batch"] == -1 and _capi._PATH_DEFAULTS["scrub_chunk"] == 0
    # reset_paths restored both: setting the defaults again is accepted, and the list of knobs names them
    _capi.set_path("scrub_batch", 1)
    _capi.set_path("scrub_chunk", 3)
    _capi.reset_paths()


def test_python_mirror_exists():
    assert callable(rs.ReedSolomon.locate_dev_batch)
    assert "rs_locate_dev_batch" in set(_capi.header_functions())


# ---------------------------------------------------------------- the confirm identity
def gf_mul(bits, a, b):
    F = leopard_np.field(bits)
    if a == 0 or b == 0:
        return 0
    return int(F.mul_log(np.array([a], np.int64), int(F._log[b]))[0])


def generator(bits, k, p, idx):
    out = np.zeros(p, np.uint32)
    assert _capi.lib().rs_debug_generator(bits, k, p, idx, out.ctypes.data) == 0
    return [int(x) for x in out]


def locate(bits, k, p, e0, e1):
    shard, scale = C.c_int(-7), C.c_uint32(7)
    assert _capi.lib().rs_debug_locate(bits, k, p, int(e0), int(e1), C.byref(shard), C.byref(scale)) == 0
    return shard.value, scale.value


def confirms(bits, p, g, scale, e):
    """The kernel's test at one symbol: e_i == G[i][j] * (scale * e_0) for every parity row i."""
    t = gf_mul(bits, int(e[0]), scale)
    return all(int(e[i]) == gf_mul(bits, g[i], t) for i in range(p))


@pytest.mark.parametrize("bits,k,p", GEOMS)
def test_confirm_identity_against_the_oracle(bits, k, p):
    S = 64
    nsym = S // 2 if bits == 16 else S
    rng = np.random.default_rng(bits * 7001 + k * 313 + p)
    data = rng.integers(0, 256, (k, S), dtype=np.uint8)
    sym = leopard_np.to_symbols(data, bits)
    par = leopard_np.to_symbols(orc.encode(bits, k, p, data), bits)

    def syndrome(changes):
        s = sym.copy()
        for j, col, diff in changes:
            s[j, col] ^= diff
        return leopard_np.to_symbols(orc.encode(bits, k, p, leopard_np.from_symbols(s, bits)), bits) ^ par

    for j in sorted({0, k // 2, k - 1}):
        col = int(rng.integers(0, nsym))
        diff = int(rng.integers(1, 1 << bits))
        e = syndrome([(j, col, diff)])
        g = generator(bits, k, p, j)
        if p == 1:
            assert locate(bits, k, p, e[0, col], 0) == (-1, 0), "p == 1: no candidate reaches the confirm"
            continue
        shard, scale = locate(bits, k, p, e[0, col], e[1, col])
        assert shard == j
        assert gf_mul(bits, g[0], scale) == 1, "row 0 of the check: G[0][j] * scale == 1"
        assert confirms(bits, p, g, scale, e[:, col]), f"{bits} {k}+{p}: one corrupt row {j} must confirm"
        assert not np.delete(e, col, axis=1).any()
        if k < 2:
            continue
        # a second corrupt data row at the same symbol: neither row explains the syndrome
        j2 = (j + 1 + int(rng.integers(0, k - 1))) % k
        e2 = syndrome([(j, col, diff), (j2, col, int(rng.integers(1, 1 << bits)))])[:, col]
        for cand in (j, j2):
            gc = generator(bits, k, p, cand)
            inv0 = locate(bits, k, p, gc[0], gc[1])[1]  # 1 / G[0][cand]
            assert gf_mul(bits, gc[0], inv0) == 1
            assert not confirms(bits, p, gc, inv0, e2), f"{bits} {k}+{p}: rows {j},{j2} confirmed as {cand}"
        # and whatever column the ratio names (if any), p >= 3 rows refute it
        shard, scale = locate(bits, k, p, e2[0], e2[1])
        if shard >= 0 and p >= 3:
            assert not confirms(bits, p, generator(bits, k, p, shard), scale, e2)
