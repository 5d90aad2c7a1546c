"""CPU tests of rs_reconstruct_dev_batch_patterns' error rules, which are all
decided before any device call (so this file runs on a machine without a GPU,
as test_rows_cpu.py does), and of the Python mirror's argument checks.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from reedsolomon16_amd import _capi

FAKE = 0x10000  # a non-NULL "device pointer": every call below must return before it is used
INV, TOO_FEW, NO_DATA, BAD_SIZE, PANIC = 53, 3, 4, 6, 50
K, P, N = 4, 2, 6
S = 128

ALL = [1] * N
ONE = [1, 1, 0, 1, 1, 1]          # a data row missing
PARITY = [1, 1, 1, 1, 1, 0]       # a parity row missing
FEW = [1, 0, 0, 1, 1, 0]          # three rows present
NONE = [0] * N


def table(*rows):
    flat = [x for r in rows for x in r]
    return (C.c_uint8 * len(flat))(*flat)


def of(*idx):
    return (C.c_uint32 * max(len(idx), 1))(*idx)


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(K, P)
    multi = rs.New16(K, P, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def call(c, base=FAKE, rs_=S, ss=N * S, ns=2, present=None, npat=2, pattern_of=None, size=S, recover_all=1):
    present = table(ONE, PARITY) if present is None else present
    pattern_of = of(0, 1) if pattern_of is None else pattern_of
    return _capi.lib().rs_reconstruct_dev_batch_patterns(c, base, rs_, ss, ns, present, npat, pattern_of, size,
                                                         recover_all, None)


def test_error_rules_in_order(codecs):
    one, multi = codecs
    h = one._h
    # NULL arguments, the stripe count, a multi-device codec
    assert _capi.lib().rs_reconstruct_dev_batch_patterns(None, FAKE, S, N * S, 2, table(ONE, PARITY), 2, of(0, 1), S, 1,
                                                         None) == INV
    assert call(h, base=None) == INV
    assert _capi.lib().rs_reconstruct_dev_batch_patterns(h, FAKE, S, N * S, 2, None, 2, of(0, 1), S, 1, None) == INV
    assert _capi.lib().rs_reconstruct_dev_batch_patterns(h, FAKE, S, N * S, 2, table(ONE, PARITY), 2, None, S, 1,
                                                         None) == INV
    assert call(h, ns=1 << 31) == INV
    assert call(multi._h) == INV
    # the pattern table's size and the per-stripe pattern numbers: before the patterns are looked at
    assert call(h, npat=0, present=table(NONE)) == INV
    assert call(h, npat=65537, present=table(NONE)) == INV
    assert call(h, pattern_of=of(0, 2), present=table(NONE, NONE)) == INV
    assert call(h, pattern_of=of(2, 0), size=0) == INV
    # no data: shard_size 0, or a pattern (named by a stripe or not) without a row
    assert call(h, size=0, present=table(FEW, ONE)) == NO_DATA
    assert call(h, present=table(ONE, NONE), pattern_of=of(0, 0)) == NO_DATA
    assert call(h, present=table(FEW, NONE)) == NO_DATA
    # too few present, referenced or not, before the size and the strides
    assert call(h, present=table(ONE, FEW), size=100) == TOO_FEW
    assert call(h, present=table(ONE, FEW), pattern_of=of(0, 0), size=100, rs_=0) == TOO_FEW
    # shard size, then the strides
    assert call(h, size=100, rs_=0) == BAD_SIZE
    assert call(h, size=96, rs_=64) == BAD_SIZE
    assert call(h, rs_=S - 64) == INV
    assert call(h, ss=N * S - 64) == INV
    assert call(h, rs_=2 * S, ss=N * S) == INV


def test_one_stripe_ignores_the_stripe_stride(codecs):
    """nstripes == 1 with nothing to rebuild: RS_OK although stripe_stride is 0."""
    one, _ = codecs
    assert call(one._h, ns=1, ss=0, present=table(ALL), npat=1, pattern_of=of(0)) == 0


def test_nothing_to_rebuild_is_ok_and_launches_nothing(codecs):
    one, _ = codecs
    h = one._h
    assert call(h, ns=0) == 0
    assert call(h, ns=0, pattern_of=of()) == 0
    # nothing missing in the referenced pattern; the other one is never used
    assert call(h, present=table(ALL, ONE), pattern_of=of(0, 0)) == 0
    # only parity missing and recover_all == 0
    assert call(h, present=table(ALL, PARITY), recover_all=0) == 0
    assert call(h, present=table(PARITY, PARITY), recover_all=0) == 0
    # ... but the errors still come first
    assert call(h, ns=0, size=100) == BAD_SIZE
    assert call(h, ns=0, size=0) == NO_DATA
    assert call(h, present=table(ALL, FEW), pattern_of=of(0, 0)) == TOO_FEW
    assert call(h, present=table(ALL, ALL), rs_=S - 64) == INV


def test_panic_geometry_before_any_device_call():
    """GF(2^8) with m + k > 256: the reference's reconstruct panics."""
    k, p = 250, 14
    c = rs.New8(k, p)
    pr = [1] * (k + p)
    pr[3] = 0
    flags = (C.c_uint8 * (k + p))(*pr)
    e = _capi.lib().rs_reconstruct_dev_batch_patterns(c._h, FAKE, S, (k + p) * S, 1, flags, 1, of(0), S, 1, None)
    assert e == PANIC
    c.close()


def test_python_mirror_argument_checks():
    assert callable(rs.ReedSolomon.reconstruct_dev_batch_patterns)
    assert "rs_reconstruct_dev_batch_patterns" in _capi.header_functions()
    np.testing.assert_array_equal(np.asarray([[True, False]], dtype=bool).astype(np.uint8), [[1, 0]])


def test_pattern_knobs(paths):
    L = _capi.lib()
    for v in (0, 1, 2):
        paths("pat_tier", v)
    assert L.rs_debug_set_path(b"pat_tier", 3) == INV
    assert L.rs_debug_set_path(b"pat_tier", -1) == INV
    for v in (0, 1, 2, 256, 1 << 20):
        paths("bsdec_grid", v)
    assert L.rs_debug_set_path(b"bsdec_grid", -1) == INV
