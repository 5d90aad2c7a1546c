"""CPU tests of the incremental update's host side: the generator coefficients
(rs_debug_generator, csrc/gf_host.cpp generator_column) against the oracle,
the linear model the update kernel evaluates, and the error rules of
rs_update_dev / rs_encode_idx_dev / rs_update_dev_batch, which are all decided
before any device call.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from oracle import leopard_np, orc
from reedsolomon16_amd import _capi

GEOMS16 = [(128, 32), (37, 9), (3, 7), (2, 1), (1, 1), (1024, 256)]
GEOMS8 = [(10, 4), (100, 28), (128, 128)]
GEOMS = [(16, k, p) for k, p in GEOMS16] + [(8, k, p) for k, p in GEOMS8]


def generator(bits, k, p, idx):
    out = np.zeros(p, np.uint32)
    e = _capi.lib().rs_debug_generator(bits, k, p, idx, out.ctypes.data)
    assert e == 0, e
    return out.astype(np.int64)


def chunk_indices(k, p):
    """0, k-1, one index inside every chunk of m data rows, and the last row of
    a ragged last chunk (which is k-1)."""
    m = leopard_np.ceil_pow2(p)
    idx = {0, k - 1}
    for c in range((k + m - 1) // m):
        cnt = min(m, k - c * m)
        idx.add(c * m + (5 * c + 3) % cnt)
    return sorted(idx)


@pytest.mark.parametrize("bits,k,p", GEOMS)
def test_generator_matches_oracle_unit_stripe(bits, k, p):
    S = 64
    for idx in chunk_indices(k, p):
        data = np.zeros((k, S), np.uint8)
        data[idx, 0] = 1  # symbol 1 in column 0 (GF(2^16): low byte 0, high byte at [32] stays 0)
        par = orc.encode(bits, k, p, data)
        want = leopard_np.to_symbols(par, bits)[:, 0]
        got = generator(bits, k, p, idx)
        assert np.array_equal(got, want), f"{bits} {k}+{p} idx {idx}"
        # nothing but column 0 is touched by a unit symbol there
        assert not leopard_np.to_symbols(par, bits)[:, 1:].any()


@pytest.mark.parametrize("bits,k,p,changed", [
    (16, 128, 32, [0, 5, 31, 32, 127]), (16, 37, 9, [36, 8, 9, 20]),
    (8, 10, 4, [9, 0, 3]), (8, 100, 28, [0, 31, 32, 99]),
])
def test_linear_model(bits, k, p, changed):
    """XOR over changed j of (old_j ^ new_j) * G[i][j] == parity(old) ^ parity(new)."""
    S = 128
    F = leopard_np.field(bits)
    rng = np.random.default_rng(bits * 100000 + k * 100 + p)
    old = rng.integers(0, 256, (k, S), dtype=np.uint8)
    new = old.copy()
    for j in changed:
        new[j] = rng.integers(0, 256, S, dtype=np.uint8)
    want = leopard_np.to_symbols(orc.encode(bits, k, p, old) ^ orc.encode(bits, k, p, new), bits)
    delta = leopard_np.to_symbols(old ^ new, bits)
    acc = np.zeros_like(want)
    for j in changed:
        g = generator(bits, k, p, j)
        for i in range(p):
            if g[i]:  # a zero coefficient contributes nothing; its log is not a log
                acc[i] ^= F.mul_log(delta[j], int(F._log[g[i]]))
    assert np.array_equal(acc, want)


def test_generator_errors():
    L = _capi.lib()
    out = np.zeros(64, np.uint32)
    o = out.ctypes.data
    INV, PANIC = 53, 50
    assert L.rs_debug_generator(12, 4, 2, 0, o) == INV
    assert L.rs_debug_generator(16, 4, 2, 0, None) == INV
    assert L.rs_debug_generator(16, 0, 2, 0, o) == INV
    assert L.rs_debug_generator(16, 4, 0, 0, o) == INV
    assert L.rs_debug_generator(16, 4, 2, -1, o) == INV
    assert L.rs_debug_generator(16, 4, 2, 4, o) == INV
    # the reference's encode panics here (skew index out of range): the oracle agrees
    k, p = 250, 6
    shards = [np.zeros(64, np.uint8) for _ in range(k + p)]
    assert orc.Oracle(8, k, p).encode(shards) == PANIC
    assert L.rs_debug_generator(8, k, p, 0, o) == PANIC


# ---------------------------------------------------------------- error rules (no device call)
FAKE = 0x10000  # a non-NULL "device pointer": every call below must fail before it is used
INV, NO_DATA, BAD_SIZE = 53, 4, 6


def ptr_array(vals):
    return (C.c_void_p * len(vals))(*vals)


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(4, 2)
    multi = rs.New16(4, 2, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def test_update_dev_errors(codecs):
    one, multi = codecs
    L, h, k, n = _capi.lib(), codecs[0]._h, 4, 6
    rows = ptr_array([FAKE] * n)
    new = ptr_array([None, FAKE, None, None])
    S = 128
    assert L.rs_update_dev(None, rows, new, S, None) == INV
    assert L.rs_update_dev(h, None, new, S, None) == INV
    assert L.rs_update_dev(h, rows, None, S, None) == INV
    assert L.rs_update_dev(multi._h, rows, new, S, None) == INV
    assert L.rs_update_dev(h, ptr_array([FAKE] * 5 + [None]), new, S, None) == INV  # NULL parity pointer
    assert L.rs_update_dev(h, ptr_array([FAKE] * 4 + [None, FAKE]), new, S, None) == INV
    assert L.rs_update_dev(h, ptr_array([FAKE, None, FAKE, FAKE, FAKE, FAKE]), new, S, None) == INV  # new without old
    assert L.rs_update_dev(h, rows, new, 0, None) == NO_DATA
    assert L.rs_update_dev(h, rows, new, 100, None) == BAD_SIZE
    # no changed row: RS_OK, nothing launched (data entries may then all be NULL)
    assert L.rs_update_dev(h, ptr_array([None] * k + [FAKE, FAKE]), ptr_array([None] * k), S, None) == 0
    assert L.rs_update_dev(h, rows, ptr_array([None] * k), S, C.c_void_p(rs.codec.RS_NULL_STREAM)) == 0


def test_encode_idx_dev_errors(codecs):
    one, multi = codecs
    L, h = _capi.lib(), codecs[0]._h
    par = ptr_array([FAKE, FAKE])
    S = 128
    assert L.rs_encode_idx_dev(None, FAKE, 0, par, S, None) == INV
    assert L.rs_encode_idx_dev(h, None, 0, par, S, None) == INV
    assert L.rs_encode_idx_dev(h, FAKE, 0, None, S, None) == INV
    assert L.rs_encode_idx_dev(multi._h, FAKE, 0, par, S, None) == INV
    assert L.rs_encode_idx_dev(h, FAKE, 0, ptr_array([FAKE, None]), S, None) == INV
    assert L.rs_encode_idx_dev(h, FAKE, -1, par, S, None) == INV
    assert L.rs_encode_idx_dev(h, FAKE, 4, par, S, None) == INV
    assert L.rs_encode_idx_dev(h, FAKE, 0, par, 0, None) == NO_DATA
    assert L.rs_encode_idx_dev(h, FAKE, 0, par, 96, None) == BAD_SIZE


def test_update_dev_batch_errors(codecs):
    one, multi = codecs
    L, h = _capi.lib(), codecs[0]._h
    S = 128

    def call(c=h, base=FAKE, rs_=S, ss=6 * S, ns=2, idx=(1, 3), nidx=None, new=FAKE * 2, nrs=S, nss=2 * S, size=S):
        arr = (C.c_int * max(len(idx), 1))(*idx) if idx is not None else None
        return L.rs_update_dev_batch(c, base, rs_, ss, ns, arr, len(idx) if nidx is None else nidx, new, nrs, nss,
                                     size, None)

    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(idx=None, nidx=1) == INV
    assert call(new=None) == INV
    assert call(c=multi._h) == INV
    assert call(ns=0) == INV
    assert call(ns=-3) == INV
    assert call(idx=(4,)) == INV       # out of [0, k)
    assert call(idx=(-1,)) == INV
    assert call(idx=(1, 1)) == INV     # repeated
    assert call(idx=(0,), nidx=0) == INV
    assert call(idx=(0, 1, 2, 3, 0), nidx=5) == INV  # nidx > k
    assert call(rs_=S - 64) == INV
    assert call(nrs=S - 64) == INV
    assert call(size=0) == NO_DATA
    assert call(size=100, rs_=128, nrs=128) == BAD_SIZE


def test_panic_geometry_is_refused_before_any_device_call():
    """GF(2^8) 250+6: the reference's encode panics, so there is no generator to update with."""
    PANIC = 50
    c = rs.New8(250, 6)
    L, S = _capi.lib(), 64
    rows = ptr_array([FAKE] * 256)
    new = ptr_array([FAKE] + [None] * 249)
    assert L.rs_update_dev(c._h, rows, new, S, None) == PANIC
    assert L.rs_encode_idx_dev(c._h, FAKE, 0, ptr_array([FAKE] * 6), S, None) == PANIC
    idx = (C.c_int * 1)(3)
    assert L.rs_update_dev_batch(c._h, FAKE, S, 256 * S, 1, idx, 1, FAKE * 2, S, S, S, None) == PANIC
    c.close()


def test_reference_entry_points_still_not_supported(codecs):
    one, _ = codecs
    with pytest.raises(rs.ErrNotSupported):
        one.update([], [])
    with pytest.raises(rs.ErrNotSupported):
        one.encode_idx(None, 0, [])


def test_python_mirror_exists():
    for name in ("update_dev", "encode_idx_dev", "update_dev_batch"):
        assert callable(getattr(rs.ReedSolomon, name))
