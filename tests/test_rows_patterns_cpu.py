"""CPU tests of rs_reconstruct_rows_dev_batch_patterns' error rules, which are
all decided before any device call (so this file runs on a machine without a
GPU, as test_patterns_cpu.py does), and of the Python mirror's presence.
"""
import ctypes as C

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
WANT_ALL = [1] * N
WANT_NONE = [0] * N


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


DEFAULT = object()


def call(c, base=FAKE, rs_=S, ss=N * S, ns=2, present=DEFAULT, required=DEFAULT, npat=2, pattern_of=DEFAULT, size=S):
    present = table(ONE, PARITY) if present is DEFAULT else present
    required = table(WANT_ALL, WANT_ALL) if required is DEFAULT else required
    pattern_of = of(0, 1) if pattern_of is DEFAULT else pattern_of
    return _capi.lib().rs_reconstruct_rows_dev_batch_patterns(c, base, rs_, ss, ns, present, required, npat,
                                                              pattern_of, size, None)


@pytest.mark.parametrize("required", [DEFAULT, None], ids=["required", "null"])
def test_error_rules_in_order(codecs, required):
    """The order of rs_reconstruct_dev_batch_patterns; a non-NULL required adds
    no error of its own, so both forms give the same answers."""
    one, multi = codecs
    h = one._h

    def go(*a, **kw):
        return call(*a, required=required, **kw)

    # 1. NULL arguments, the stripe count, a multi-device codec, the table's size, the pattern numbers
    assert go(None) == INV
    assert go(h, base=None) == INV
    assert go(h, present=None) == INV
    assert go(h, pattern_of=None) == INV
    assert go(h, ns=1 << 31) == INV
    assert go(multi._h) == INV
    assert go(multi._h, size=0) == INV  # before the data rules on a multi-device codec too
    assert go(h, npat=0, present=table(NONE)) == INV
    assert go(h, npat=65537, present=table(NONE)) == INV
    assert go(h, pattern_of=of(0, 2), present=table(NONE, NONE)) == INV
    assert go(h, pattern_of=of(2, 0), size=0) == INV
    # 2. no data: shard_size 0, or a table row (named by a stripe or not) without a shard
    assert go(h, size=0, present=table(FEW, ONE)) == NO_DATA
    assert go(h, present=table(ONE, NONE), pattern_of=of(0, 0)) == NO_DATA
    assert go(h, present=table(FEW, NONE)) == NO_DATA
    # 3. too few present, referenced or not, before the size and the strides
    assert go(h, present=table(ONE, FEW), size=100) == TOO_FEW
    assert go(h, present=table(ONE, FEW), pattern_of=of(0, 0), size=100, rs_=0) == TOO_FEW
    # 4. the shard size, then 5. the strides
    assert go(h, size=100, rs_=0) == BAD_SIZE
    assert go(h, size=96, rs_=64) == BAD_SIZE
    assert go(h, rs_=S - 64) == INV
    assert go(h, ss=N * S - 64) == INV
    assert go(h, rs_=2 * S, ss=N * S) == INV


def test_the_same_rules_on_a_multi_device_codec(codecs):
    """A multi-device codec is refused at rule 1 whatever else is wrong."""
    _, multi = codecs
    m = multi._h
    for kw in (dict(), dict(size=0), dict(present=table(ONE, FEW)), dict(size=100), dict(rs_=S - 64), dict(ns=0),
               dict(present=table(ALL, ALL)), dict(required=None)):
        assert call(m, **kw) == INV


def test_too_few_is_decided_without_looking_at_required(codecs):
    """A table row with too few present is an error even where nothing of it is
    wanted: the rule is that of the patterns call."""
    one, _ = codecs
    assert call(one._h, present=table(ONE, FEW), required=table(WANT_ALL, WANT_NONE)) == TOO_FEW
    assert call(one._h, present=table(ALL, FEW), required=table(WANT_NONE, WANT_NONE), pattern_of=of(0, 0)) == TOO_FEW


def test_one_stripe_ignores_the_stripe_stride(codecs):
    one, _ = codecs
    assert call(one._h, ns=1, ss=0, present=table(ALL), required=table(WANT_ALL), npat=1, pattern_of=of(0)) == 0


def test_nothing_to_rebuild_is_ok_and_launches_nothing(codecs):
    one, _ = codecs
    h = one._h
    assert call(h, ns=0) == 0
    assert call(h, ns=0, pattern_of=of()) == 0
    assert call(h, ns=0, required=None) == 0
    # nothing missing in the referenced pair; the other one is never used
    assert call(h, present=table(ALL, ONE), pattern_of=of(0, 0)) == 0
    assert call(h, present=table(ALL, ONE), pattern_of=of(0, 0), required=None) == 0
    # rows missing, none of them required
    assert call(h, required=table(WANT_NONE, WANT_NONE)) == 0
    # a required flag on a present row is ignored: only present rows are flagged here
    assert call(h, required=table(ONE, PARITY)) == 0
    assert call(h, present=table(ALL, ALL), required=table(WANT_ALL, WANT_ALL)) == 0
    # ... but the errors still come first
    assert call(h, ns=0, size=100) == BAD_SIZE
    assert call(h, ns=0, size=0) == NO_DATA
    assert call(h, required=table(WANT_NONE, WANT_NONE), size=100) == BAD_SIZE
    assert call(h, present=table(ALL, FEW), pattern_of=of(0, 0)) == TOO_FEW
    assert call(h, present=table(ALL, ALL), rs_=S - 64) == INV


@pytest.mark.parametrize("null_required", [False, True], ids=["required", "null"])
def test_panic_geometry_before_any_device_call(null_required):
    """GF(2^8) with m + k > 256: the reference's reconstruct panics."""
    k, p = 250, 14
    c = rs.New8(k, p)
    pr = [1] * (k + p)
    pr[3] = 0
    flags = (C.c_uint8 * (k + p))(*pr)
    req = None if null_required else (C.c_uint8 * (k + p))(*([1] * (k + p)))
    L = _capi.lib()
    e = L.rs_reconstruct_rows_dev_batch_patterns(c._h, FAKE, S, (k + p) * S, 1, flags, req, 1, of(0), S, None)
    assert e == PANIC
    # after the strides, before "nothing to rebuild"
    assert L.rs_reconstruct_rows_dev_batch_patterns(c._h, FAKE, S - 64, (k + p) * S, 1, flags, req, 1, of(0), S,
                                                    None) == INV
    allp = (C.c_uint8 * (k + p))(*([1] * (k + p)))
    assert L.rs_reconstruct_rows_dev_batch_patterns(c._h, FAKE, S, (k + p) * S, 1, allp, req, 1, of(0), S, None) == PANIC
    c.close()


def test_python_mirror():
    assert callable(rs.ReedSolomon.reconstruct_rows_dev_batch_patterns)
    assert "rs_reconstruct_rows_dev_batch_patterns" in _capi.header_functions()
