"""CPU tests of the scrub's host side: the ratio map that names a corrupt data
shard from two syndrome symbols (rs_debug_locate, csrc/gf_host.cpp
make_locate_map) against the oracle, the rows of G it is built from, and the
error rules of rs_verify_dev_batch_map / rs_locate_dev / rs_scrub_dev_batch,
which are all decided before any device call.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from oracle import leopard_np, orc
from reedsolomon16_amd import _capi

# test_update_cpu.py's geometries plus 5+2
GEOMS16 = [(128, 32), (37, 9), (3, 7), (2, 1), (1, 1), (1024, 256), (5, 2)]
GEOMS8 = [(10, 4), (100, 28), (128, 128)]
GEOMS = [(16, k, p) for k, p in GEOMS16] + [(8, k, p) for k, p in GEOMS8]


def locate(bits, k, p, e0, e1):
    shard, scale = C.c_int(-7), C.c_uint32(7)
    e = _capi.lib().rs_debug_locate(bits, k, p, int(e0), int(e1), C.byref(shard), C.byref(scale))
    assert e == 0, e
    return shard.value, scale.value


def generator(bits, k, p, idx):
    out = np.zeros(p, np.uint32)
    assert _capi.lib().rs_debug_generator(bits, k, p, idx, out.ctypes.data) == 0
    return out.astype(np.int64)


def chunk_indices(k, p):
    """0, k-1 and one index inside every chunk of m data rows."""
    m = leopard_np.ceil_pow2(p)
    idx = {0, k - 1}
    for c in range((k + m - 1) // m):
        cnt = min(m, k - c * m)
        idx.add(c * m + (5 * c + 3) % cnt)
    return sorted(idx)


def gf_mul(bits, a, b):
    F = leopard_np.field(bits)
    if a == 0 or b == 0:
        return 0
    return int(F.mul_log(np.array([a], np.int64), int(F._log[b]))[0])


@pytest.mark.parametrize("bits,k,p", GEOMS)
def test_ratio_map_names_the_corrupt_shard(bits, k, p):
    """One random symbol XORed into data row j of an oracle-encoded stripe: the
    syndrome symbols of parity rows 0 and 1 name j, and scale * e0 is the
    injected difference."""
    S = 64
    nsym = S // 2 if bits == 16 else S
    rng = np.random.default_rng(bits * 100003 + k * 101 + p)
    data = rng.integers(0, 256, (k, S), dtype=np.uint8)
    par = leopard_np.to_symbols(orc.encode(bits, k, p, data), bits)
    for j in chunk_indices(k, p):
        col = int(rng.integers(0, nsym))
        diff = int(rng.integers(1, 1 << bits))
        sym = leopard_np.to_symbols(data, bits).copy()
        sym[j, col] ^= diff
        bad = leopard_np.from_symbols(sym, bits)
        e = leopard_np.to_symbols(orc.encode(bits, k, p, bad), bits) ^ par
        assert e[:, col].all(), "every entry of G is non-zero: every parity row differs there"
        assert not np.delete(e, col, axis=1).any()
        if p == 1:  # one syndrome row cannot tell the shards apart
            assert locate(bits, k, p, e[0, col], 0) == (-1, 0)
            assert locate(bits, k, p, e[0, col], e[0, col]) == (-1, 0)
            continue
        shard, scale = locate(bits, k, p, e[0, col], e[1, col])
        assert shard == j, f"{bits} {k}+{p}: shard {j} located as {shard}"
        assert gf_mul(bits, int(e[0, col]), scale) == diff


@pytest.mark.parametrize("bits,k,p", [(16, 5, 2), (16, 37, 9), (8, 10, 4)])
def test_no_matching_column(bits, k, p):
    F = leopard_np.field(bits)
    ratios = set()
    for j in range(k):
        g = generator(bits, k, p, j)
        inv0 = int(F._exp[(F.mod - int(F._log[g[0]])) % F.mod])
        ratios.add(gf_mul(bits, int(g[1]), inv0))
    assert len(ratios) == k, "the k ratios are pairwise distinct"
    free = next(r for r in range(1, 1 << bits) if r not in ratios)
    assert locate(bits, k, p, 1, free) == (-1, 0)  # e1 / 1 = free: no column
    assert locate(bits, k, p, 0, 5) == (-1, 0)     # a zero syndrome symbol is no data shard's
    assert locate(bits, k, p, 5, 0) == (-1, 0)
    hit = sorted(ratios)[0]
    shard, scale = locate(bits, k, p, 1, hit)
    assert 0 <= shard < k and scale != 0
    if bits == 8:
        assert locate(bits, k, p, 1, 256) == (-1, 0)  # not a symbol of the field


@pytest.mark.parametrize("bits,k,p", [g for g in GEOMS if g[2] >= 2])
def test_generator_rows_from_decode_coefficients(bits, k, p):
    """Rows 0 and 1 of G as the map takes them (the decode map of "every parity
    shard erased") equal rs_debug_generator's columns."""
    L = _capi.lib()
    present = (C.c_uint8 * (k + p))(*([1] * k + [0] * p))
    rows = []
    for i in range(2):
        out = np.zeros(k + p, np.uint32)
        assert L.rs_debug_decode_coefficients(bits, k, p, present, k + i, out.ctypes.data) == 0
        assert not out[k:].any()
        rows.append(out.astype(np.int64))
    for j in chunk_indices(k, p):
        g = generator(bits, k, p, j)
        assert (rows[0][j], rows[1][j]) == (g[0], g[1]), f"{bits} {k}+{p} column {j}"


def test_debug_locate_errors():
    L = _capi.lib()
    shard, scale = C.c_int(0), C.c_uint32(0)
    INV, PANIC = 53, 50
    assert L.rs_debug_locate(12, 4, 2, 1, 1, C.byref(shard), C.byref(scale)) == INV
    assert L.rs_debug_locate(16, 0, 2, 1, 1, C.byref(shard), C.byref(scale)) == INV
    assert L.rs_debug_locate(16, 4, 0, 1, 1, C.byref(shard), C.byref(scale)) == INV
    assert L.rs_debug_locate(16, 4, 2, 1, 1, None, C.byref(scale)) == INV
    assert L.rs_debug_locate(16, 4, 2, 1, 1, C.byref(shard), None) == INV
    assert L.rs_debug_locate(8, 250, 6, 1, 1, C.byref(shard), C.byref(scale)) == PANIC  # the encode panics


# ---------------------------------------------------------------- error rules (no device call)
FAKE = 0x10000  # a non-NULL "device pointer": every call below must fail before it is used
INV, NO_DATA, BAD_SIZE, PANIC = 53, 4, 6, 50


def ptr_array(vals):
    return (C.c_void_p * len(vals))(*vals)


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(4, 2)
    multi = rs.New16(4, 2, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def test_verify_dev_batch_map_errors(codecs):
    one, multi = codecs
    L, h, S = _capi.lib(), codecs[0]._h, 128
    bad = (C.c_uint8 * 4)()
    nbad = C.c_int(9)

    def call(c=h, base=FAKE, rs_=S, ss=6 * S, ns=2, size=S, b=bad, nb=C.byref(nbad)):
        return L.rs_verify_dev_batch_map(c, base, rs_, ss, ns, size, b, nb, None)

    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(b=None) == INV
    assert call(ns=0) == INV
    assert call(ns=-1) == INV
    assert call(c=multi._h) == INV
    assert call(size=0) == NO_DATA
    assert call(size=100) == BAD_SIZE
    assert call(size=0, rs_=0) == NO_DATA       # the size rules come before the stride rule
    assert call(size=192, rs_=100) == INV       # row_stride < shard_size
    assert call(size=100, rs_=64) == BAD_SIZE
    assert call(size=0, nb=None) == NO_DATA     # nbad is optional


def test_locate_dev_errors(codecs):
    one, multi = codecs
    L, h, S = _capi.lib(), codecs[0]._h, 128
    rows = ptr_array([FAKE] * 6)
    v = C.c_int(5)
    assert L.rs_locate_dev(None, rows, S, 0, C.byref(v), None) == INV
    assert L.rs_locate_dev(h, None, S, 0, C.byref(v), None) == INV
    assert L.rs_locate_dev(h, rows, S, 0, None, None) == INV
    assert L.rs_locate_dev(multi._h, rows, S, 0, C.byref(v), None) == INV
    assert L.rs_locate_dev(h, ptr_array([FAKE] * 5 + [None]), S, 1, C.byref(v), None) == INV
    assert L.rs_locate_dev(h, ptr_array([None] + [FAKE] * 5), S, 1, C.byref(v), None) == INV
    assert L.rs_locate_dev(h, rows, 0, 0, C.byref(v), None) == NO_DATA
    assert L.rs_locate_dev(h, rows, 100, 1, C.byref(v), None) == BAD_SIZE
    assert L.rs_locate_dev(h, ptr_array([None] * 6), 0, 0, C.byref(v), None) == INV  # NULL rows before the size


def test_scrub_dev_batch_errors(codecs):
    one, multi = codecs
    L, h, S = _capi.lib(), codecs[0]._h, 128
    verdict = (C.c_int32 * 4)()
    nbad = C.c_int(9)

    def call(c=h, base=FAKE, rs_=S, ss=6 * S, ns=2, size=S, repair=0, v=verdict, nb=C.byref(nbad)):
        return L.rs_scrub_dev_batch(c, base, rs_, ss, ns, size, repair, v, nb, None)

    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(v=None) == INV
    assert call(ns=0) == INV
    assert call(c=multi._h, repair=1) == INV
    assert call(size=0) == NO_DATA
    assert call(size=96, repair=1) == BAD_SIZE
    assert call(size=192, rs_=128) == INV
    assert call(size=0, nb=None) == NO_DATA


def test_panic_geometry_is_refused_before_any_device_call():
    """GF(2^8) 250+6: the reference's encode panics, so there is no parity to recompute."""
    c = rs.New8(250, 6)
    L, S = _capi.lib(), 64
    v = C.c_int(0)
    bad = (C.c_uint8 * 1)()
    verdict = (C.c_int32 * 1)()
    assert L.rs_locate_dev(c._h, ptr_array([FAKE] * 256), S, 0, C.byref(v), None) == PANIC
    assert L.rs_verify_dev_batch_map(c._h, FAKE, S, 256 * S, 1, S, bad, None, None) == PANIC
    assert L.rs_scrub_dev_batch(c._h, FAKE, S, 256 * S, 1, S, 1, verdict, None, None) == PANIC
    c.close()


def test_python_mirror_exists():
    for name in ("verify_dev_batch_map", "locate_dev", "scrub_dev_batch"):
        assert callable(getattr(rs.ReedSolomon, name))
    assert (rs.SCRUB_CLEAN, rs.SCRUB_UNLOCATED) == (-1, -2)
    assert {"rs_verify_dev_batch_map", "rs_locate_dev", "rs_scrub_dev_batch", "rs_debug_locate"} <= set(
        _capi.header_functions())
