"""CPU tests of rs_reconstruct_rows_checked_dev_batch_patterns' host side
(DESIGN.md 4.19): the check weights (rs_debug_check_weights) against oracle
codewords -- the weighted sum over the rows marked present vanishes, a single
changed survivor shows in check 0 exactly where it changed, and a pair built to
cancel check 0 shows in check 1 -- and the call's error table, decided before
any device call.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from oracle import leopard_np
from reedsolomon16_amd import _capi
from tests.checked_util import codeword
from tests.scrub_set_util import gf_mul
from tests.test_checked_cpu import COLUMN_CASES, missing_rows, present_flags

FAKE = 0x10000  # a non-NULL "device pointer": every call below must return before it is used
OK, INV, NO_DATA, TOO_FEW, BAD_SIZE, PANIC = 0, 53, 4, 3, 6, 50
S = 64

WEIGHT_CASES = COLUMN_CASES + [(8, 128, 128, 1), (8, 128, 128, 2)]


def check_weights(bits, k, p, present, l):
    out = np.full(k + p, 0xDEAD, np.uint32)
    err = _capi.lib().rs_debug_check_weights(bits, k, p, present.ctypes.data_as(C.POINTER(C.c_uint8)), l, out.ctypes.data)
    assert err == OK, err
    return out.astype(np.int64)


def positions(k, p):
    """Shard t's position: parity shard i at i, data shard j at ceil_pow2(p) + j."""
    m = leopard_np.ceil_pow2(p)
    return np.array([m + t if t < k else t - k for t in range(k + p)], np.int64)


def gf_inv(bits, a):
    F = leopard_np.field(bits)
    return F._exp[F.sub_mod(0, F._log[np.asarray(a, np.int64)])]


def check_sum(bits, h, sym):
    """sum over the shards of h[t] * row t, per symbol."""
    return np.bitwise_xor.reduce(gf_mul(bits, h[:, None], sym), axis=0)


@pytest.mark.parametrize("bits,k,p,e", WEIGHT_CASES)
def test_check_weights(bits, k, p, e):
    good, rng = codeword(bits, k, p, S, bits * 307 + k * 11 + p * 3 + e)
    E = missing_rows(k, p, e, rng)
    pr = present_flags(k, p, E)
    assert k + p - e - k >= 2, "two checks exist"
    h0, h1 = check_weights(bits, k, p, pr, 0), check_weights(bits, k, p, pr, 1)
    present = np.flatnonzero(pr)
    assert not h0[E].any() and not h1[E].any(), "0 at the shards not present"
    assert h0[present].all(), "check 0 sees every present shard"
    x = positions(k, p)
    assert np.array_equal(h1, gf_mul(bits, h0, x)), "h_1[t] = h_0[t] * x_t"
    sym = leopard_np.to_symbols(good, bits)
    garbage = sym.copy()
    garbage[E] = rng.integers(0, 1 << bits, (len(E), sym.shape[1]))  # a missing row's content has weight 0
    for h in (h0, h1):
        assert not check_sum(bits, h, garbage).any(), f"GF(2^{bits}) {k}+{p}, E = {E}"
    # one survivor changed at some symbols: check 0 is non-zero exactly there
    for t in (0, k - 1, k, k + 2):
        bad = sym.copy()
        where = np.sort(rng.choice(sym.shape[1], 5, replace=False))
        bad[t, where] ^= rng.integers(1, 1 << bits, 5)
        got = check_sum(bits, h0, bad)
        assert np.array_equal(np.flatnonzero(got), where), f"t = {t}"
    # two survivors changed so that check 0 cancels: check 1 does not
    for a, b in ((0, k - 1), (k, 0), (k + 2, k)):
        bad = sym.copy()
        Da = int(rng.integers(1, 1 << bits))
        Db = int(gf_mul(bits, gf_mul(bits, Da, h0[a]), gf_inv(bits, h0[b])))
        bad[a, 3] ^= Da
        bad[b, 3] ^= Db
        assert not check_sum(bits, h0, bad).any(), (a, b)
        assert np.array_equal(np.flatnonzero(check_sum(bits, h1, bad)), [3]), (a, b)


def test_debug_errors():
    L = _capi.lib()
    pr = np.ones(14, np.uint8)
    pr[3] = 0
    prp = pr.ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.zeros(14, np.uint32)
    for l in (0, 1, 2):
        assert L.rs_debug_check_weights(16, 10, 4, prp, l, out.ctypes.data) == OK
    assert L.rs_debug_check_weights(16, 10, 4, prp, 3, out.ctypes.data) == INV, "13 present: three checks"
    assert L.rs_debug_check_weights(16, 10, 4, prp, -1, out.ctypes.data) == INV
    assert L.rs_debug_check_weights(12, 10, 4, prp, 0, out.ctypes.data) == INV
    assert L.rs_debug_check_weights(16, 10, 4, None, 0, out.ctypes.data) == INV
    assert L.rs_debug_check_weights(16, 10, 4, prp, 0, None) == INV
    assert L.rs_debug_check_weights(16, 0, 4, prp, 0, out.ctypes.data) == INV
    big = np.ones(256, np.uint8)
    o2 = np.zeros(256, np.uint32)
    assert L.rs_debug_check_weights(8, 250, 6, big.ctypes.data_as(C.POINTER(C.c_uint8)), 0, o2.ctypes.data) == PANIC


# ---------------------------------------------------------------- the error table
def u32(vals):
    return (C.c_uint32 * max(len(vals), 1))(*vals)


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(4, 2)
    multi = rs.New16(4, 2, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def test_rows_checked_errors(codecs):
    one, multi = codecs
    L, h = _capi.lib(), one._h
    verdict = (C.c_int32 * 4)(7, 7, 7, 7)
    nbad = C.c_int(9)
    BIG = 1 << 31
    table = np.array([[1, 1, 1, 1, 1, 0], [0, 1, 1, 1, 1, 1]], np.uint8)
    req = np.ones((2, 6), np.uint8)

    def call(c=h, base=FAKE, rs_=128, ss=6 * 128, ns=4, tab=table, rq=req, npat=None, of=(0, 1, 1, 0), size=128, checks=2,
             vd=verdict, nb=nbad, notab=False, noof=False):
        t = None if notab else np.ascontiguousarray(tab).ctypes.data_as(C.POINTER(C.c_uint8))
        r = None if rq is None else np.ascontiguousarray(rq).ctypes.data_as(C.POINTER(C.c_uint8))
        return L.rs_reconstruct_rows_checked_dev_batch_patterns(
            c, base, rs_, ss, ns, t, r, len(tab) if npat is None else npat, None if noof else u32(of), size, checks, vd,
            C.byref(nb) if nb is not None else None, None)

    # RS_ERR_INVALID_ARG: the NULL arguments, verdict among them, the counts, the codec
    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(notab=True) == INV
    assert call(noof=True) == INV
    assert call(vd=None) == INV
    assert call(ns=BIG) == INV
    assert call(c=multi._h) == INV
    assert call(npat=0) == INV
    assert call(npat=65537) == INV
    assert nbad.value == 9, "an argument error touched *nbad"
    # the table, in rs_reconstruct_rows_dev_batch_patterns' order; required may be NULL
    for rq in (req, None):
        assert call(of=(0, 2, 0, 0), rq=rq) == INV
        assert call(of=(0, 2, 0, 0), size=0, rq=rq) == INV
        assert call(size=0, rq=rq) == NO_DATA
        none = np.array([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]], np.uint8)
        assert call(tab=none, rq=rq) == NO_DATA
        few = np.array([[1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1]], np.uint8)
        assert call(tab=few, rq=rq) == TOO_FEW
        assert call(tab=few, size=100, rq=rq) == TOO_FEW
        assert call(size=100, rq=rq) == BAD_SIZE
        assert call(size=192, rs_=128, rq=rq) == INV
        assert call(ss=5 * 128, rq=rq) == INV
    assert nbad.value == 0
    # checks comes after the table
    assert call(checks=-1) == INV
    assert call(checks=3) == INV
    assert call(checks=3, size=0) == NO_DATA
    assert call(checks=-1, tab=few) == TOO_FEW
    assert call(checks=3, size=100) == BAD_SIZE
    assert call(vd=None, size=0) == INV
    assert list(verdict) == [7] * 4, "an error wrote a verdict"
    # no stripe: served without a device call, for every check count
    for checks in (0, 1, 2):
        assert call(ns=0, of=(), checks=checks) == OK
    assert list(verdict) == [7] * 4
    # checks == 0 and nothing to rebuild: NONE everywhere, no device call
    allp = np.ones((2, 6), np.uint8)
    assert call(tab=allp, checks=0) == OK
    assert list(verdict) == [2] * 4 and nbad.value == 0


def test_panic_geometry_is_refused_before_any_device_call():
    c = rs.New8(250, 6)
    L = _capi.lib()
    verdict = (C.c_int32 * 2)()
    table = np.ones((1, 256), np.uint8)
    table[0, 3] = 0
    assert L.rs_reconstruct_rows_checked_dev_batch_patterns(
        c._h, FAKE, S, 256 * S, 2, table.ctypes.data_as(C.POINTER(C.c_uint8)), None, 1, u32([0, 0]), S, 2, verdict, None,
        None) == PANIC
    c.close()


def test_python_mirror_exists():
    assert callable(rs.ReedSolomon.reconstruct_rows_checked_dev_batch_patterns)
    assert (rs.ROWS_CHECK_OK, rs.ROWS_CHECK_BAD, rs.ROWS_CHECK_NONE, rs.ROWS_CHECKS_MAX) == (0, 1, 2, 2)
    assert {"rs_reconstruct_rows_checked_dev_batch_patterns", "rs_debug_check_weights"} <= set(_capi.header_functions())
