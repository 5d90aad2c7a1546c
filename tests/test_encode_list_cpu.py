"""CPU tests of rs_encode_dev_list's / rs_verify_dev_list's host side: the error
rules, all decided before any device call (on codecs that never touch a
device, with fake device pointers, so every call below must fail or launch
nothing), the span bound (rs_debug_encode_list_fits), the launch plan the
call would make (rs_debug_encode_list_plan) and the Python mirror's type
checks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from reedsolomon16_amd import _capi

FAKE = 0x10000  # a non-NULL "device pointer": never dereferenced here
INV, NO_DATA, BAD_SIZE, PANIC = 53, 4, 6, 50
K, P = 4, 2
GOOD = (FAKE, 128, 128)


def stripe_array(stripes):
    arr = (_capi.Stripe * max(len(stripes), 1))()
    for i, (b, st, S) in enumerate(stripes):
        arr[i] = _capi.Stripe(b, st, S)
    return arr


def enc(h, stripes, n=None, null_list=False):
    L = _capi.lib()
    return L.rs_encode_dev_list(h, None if null_list else stripe_array(stripes), len(stripes) if n is None else n, None)


def ver(h, stripes, n=None, null_list=False, null_ok=False, verdict=True):
    """(code, ok, verdicts)"""
    L = _capi.lib()
    cnt = len(stripes) if n is None else n
    v = np.full(max(len(stripes), 1), 7, np.int8)
    ok = C.c_int(7)
    code = L.rs_verify_dev_list(h, None if null_list else stripe_array(stripes), cnt, v.ctypes.data if verdict else None,
                                None if null_ok else C.byref(ok), None)
    return code, ok.value, v


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(K, P)
    multi = rs.New16(K, P, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def both(h, stripes, **kw):
    """The code of the encode and of the verify form, which must agree."""
    a, b = enc(h, stripes, **kw), ver(h, stripes, **kw)[0]
    assert a == b
    return a


# a stripe that breaks exactly one rule, by rule number
NULL_BASE = (None, 128, 128)                      # 1
NO_BYTES = (FAKE, 128, 0)                         # 2
ODD = (FAKE, 128, 100)                            # 3
SHORT_STRIDE = (FAKE, 64, 128)                    # 4
WIDE_SPAN = (FAKE, 1 << 31, 128)                  # 5: 3 * 2^31 + 128 >= 2^32


def test_each_rule(codecs):
    h = codecs[0]._h
    assert both(None, [GOOD]) == INV
    assert both(h, [GOOD], null_list=True) == INV
    assert ver(h, [GOOD], null_ok=True)[0] == INV
    assert both(h, [GOOD], n=2**31) == INV  # decided before the list is read
    assert both(h, [GOOD, NULL_BASE]) == INV
    assert both(h, [GOOD, NO_BYTES]) == NO_DATA
    assert both(h, [GOOD, ODD]) == BAD_SIZE
    assert both(h, [SHORT_STRIDE, GOOD]) == INV
    assert both(h, [GOOD, WIDE_SPAN, GOOD]) == INV
    # a failing verify says not ok
    assert ver(h, [GOOD, ODD])[1] == 0


def test_rule_order(codecs):
    """Each rule is applied to the whole list before the next: an earlier rule
    broken by a later stripe wins over a later rule broken by an earlier one."""
    h = codecs[0]._h
    assert both(h, [NO_BYTES, NULL_BASE]) == INV          # 1 before 2
    assert both(h, [ODD, NO_BYTES]) == NO_DATA            # 2 before 3
    assert both(h, [SHORT_STRIDE, ODD]) == BAD_SIZE       # 3 before 4
    assert both(h, [(FAKE, 64, 100)]) == BAD_SIZE         # ... in one stripe
    assert both(h, [(FAKE, 0, 0)]) == NO_DATA
    assert both(h, [WIDE_SPAN, NO_BYTES]) == NO_DATA      # 2 before 5
    assert both(h, [WIDE_SPAN, ODD]) == BAD_SIZE          # 3 before 5
    # 4 and 5 give the same code; 6 comes after both
    panics = rs.New8(250, 6)                              # 8 + 250 > 256: the reference's encode panics
    try:
        hp = panics._h
        assert both(hp, [GOOD]) == PANIC
        assert both(hp, [GOOD, SHORT_STRIDE]) == INV      # 4 before 6
        assert both(hp, [WIDE_SPAN, GOOD]) == INV         # 5 before 6
        assert both(hp, [GOOD, ODD]) == BAD_SIZE
        assert both(hp, [GOOD, NO_BYTES]) == NO_DATA
        assert both(hp, []) == PANIC                      # the geometry is refused even with nothing to do
    finally:
        panics.close()


def test_multi_device_codec_is_refused(codecs):
    h = codecs[1]._h
    assert both(h, [GOOD]) == INV
    assert both(h, []) == INV
    assert both(h, [NO_BYTES]) == INV   # rule 1 comes first
    assert both(h, [ODD]) == INV


def test_no_stripes(codecs):
    h = codecs[0]._h
    assert enc(h, []) == 0
    code, ok, _ = ver(h, [])
    assert (code, ok) == (0, 1)
    assert ver(h, [], verdict=False)[:2] == (0, 1)
    assert enc(h, [NO_BYTES], n=0) == 0  # nothing is read
    # ... and nothing was launched: the codec still has no device half, so a
    # call that needed one would have failed where there is no device
    assert codecs[0].encode_dev_list([], stream=0) is None
    assert codecs[0].verify_dev_list([], stream=0).shape == (0,)


@pytest.mark.parametrize("k", [2, 4, 10, 37, 128])
@pytest.mark.parametrize("S", [64, 8256, 1 << 20])
def test_span_bound(k, S):
    """Rule 5 at its last fitting stride and 64 bytes beyond: (k-1) * stride + S < 2^32."""
    L = _capi.lib()
    last = ((1 << 32) - 1 - S) // (k - 1) // 64 * 64   # the last multiple of 64 that fits
    assert (k - 1) * last + S < 1 << 32 <= (k - 1) * (last + 64) + S
    assert L.rs_debug_encode_list_fits(k, last, S) == 1
    assert L.rs_debug_encode_list_fits(k, last + 64, S) == 0
    assert L.rs_debug_encode_list_fits(k, S, S) == 1
    assert L.rs_debug_encode_list_fits(k, 2**64 - 64, S) == 0   # the product wraps
    assert L.rs_debug_encode_list_fits(k, 1 << 62, S) == 0
    c = rs.New16(k, 2)
    try:
        # refused by the call itself (the stride that fits is not called: the pointer is fake)
        assert both(c._h, [GOOD, (FAKE, last + 64, S)]) == INV
    finally:
        c.close()
    assert L.rs_debug_encode_list_fits(1, 1 << 40, S) == 1      # one data row: no stride enters
    assert L.rs_debug_encode_list_fits(1, S, 1 << 32) == 0
    assert L.rs_debug_encode_list_fits(1, S, (1 << 32) - 64) == 1


# ---------------------------------------------------------------- the plan
def plan(bits, p, uw, sizes, max_stripes=0):
    """[(z0, z1, wg_bytes, nwg, first_wg array)] or the error code."""
    L = _capi.lib()
    sz = (C.c_size_t * max(len(sizes), 1))(*sizes)
    nl = C.c_int(-1)
    code = L.rs_debug_encode_list_plan(bits, p, uw, sz, len(sizes), max_stripes, C.byref(nl), None, None)
    if code:
        return code
    launches = np.zeros(4 * max(nl.value, 1), np.uint64)
    fw = np.zeros(len(sizes) + nl.value + 1, np.uint32)
    assert L.rs_debug_encode_list_plan(bits, p, uw, sz, len(sizes), max_stripes, C.byref(nl), launches.ctypes.data,
                                       fw.ctypes.data) == 0
    out, at = [], 0
    for i in range(nl.value):
        z0, z1, wg, nwg = (int(x) for x in launches[4 * i:4 * i + 4])
        out.append((z0, z1, wg, nwg, fw[at:at + z1 - z0 + 1].copy()))
        at += z1 - z0 + 1
    return out


def find(fw, wg):
    """The kernel's search (gf_host.hpp encode_list_find)."""
    lo, hi = 0, len(fw) - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if fw[mid] <= wg:
            lo = mid
        else:
            hi = mid
    return lo


NINE = [64, 192, 1024, 1088, 4096, 4160, 8192, 8256, 64]
# (bits, p) -> (wide, narrow or None): bytes of a row per workgroup of the register encode
UNITS = {(8, 1): (4096, None), (8, 4): (4096, 1024), (8, 7): (4096, 1024), (8, 16): (4096, 1024), (8, 28): (2048, None),
         (16, 1): (8192, None), (16, 7): (8192, None), (16, 9): (4096, None), (16, 32): (2048, None)}


def check_plan(pl, sizes, wg_want, max_stripes=None, step=1):
    at = 0
    for z0, z1, wg, nwg, fw in pl:
        assert z0 == at and z1 > z0
        at = z1
        assert wg == wg_want
        if max_stripes:
            assert z1 - z0 <= max_stripes
        blocks = [-(-s // wg) for s in sizes[z0:z1]]
        np.testing.assert_array_equal(fw, np.concatenate([[0], np.cumsum(blocks)]))
        assert nwg == fw[-1] < 2**31
        for i in sorted(set(range(0, len(blocks), step)) | {len(blocks) - 1}):
            b = blocks[i]
            for blk in {0, b // 2, b - 1}:
                assert find(fw, int(fw[i]) + blk) == i
    assert at == len(sizes)


@pytest.mark.parametrize("geom", sorted(UNITS))
def test_plan_both_unit_widths(geom):
    bits, p = geom
    wide, narrow = UNITS[geom]
    rng = np.random.default_rng(5)
    ragged = [int(x) * 64 for x in rng.integers(1, 600, 500)]
    for sizes in (NINE, ragged):
        pl = plan(bits, p, 0, sizes)
        assert len(pl) == 1
        check_plan(pl, sizes, wide)
        pl = plan(bits, p, 1, sizes)
        check_plan(pl, sizes, narrow or wide)
        # a cut by stripe count
        pl = plan(bits, p, 0, sizes, max_stripes=4)
        assert len(pl) == -(-len(sizes) // 4)
        check_plan(pl, sizes, wide, 4)
    # automatic: the narrow unit below 1024 wide workgroups in the launch, as the register encode picks it
    small = [4096] * 1023
    if narrow:
        check_plan(plan(bits, p, -1, small), small, narrow)
    else:
        check_plan(plan(bits, p, -1, small), small, wide)
    large = [wide] * 1024
    check_plan(plan(bits, p, -1, large), large, wide)


def test_plan_ring_slot_cut():
    """The library's own limit: descriptors and prefix of a launch fit one 4 MiB ring slot."""
    sizes = [64] * 200_001
    pl = plan(16, 1, -1, sizes)
    assert len(pl) == 2
    z0, z1, wg, nwg, fw = pl[0]
    assert 256 + 24 * (z1 - z0) + 4 * (z1 - z0 + 1) <= 4 << 20 < 256 + 28 * (z1 - z0 + 1) + 4
    check_plan(pl, sizes, 8192, step=997)


def test_plan_workgroup_cut():
    """A launch is cut before its workgroup count reaches 2^31.  Sizes only:
    2^32 - 64 bytes in 1024-byte workgroups are 2^22 workgroups a stripe, so
    511 stripes fit a launch and the 512th does not."""
    sizes = [(1 << 32) - 64] * 1200
    pl = plan(8, 4, 1, sizes)
    assert [(z0, z1, nwg) for z0, z1, _, nwg, _ in pl] == [(0, 511, 511 << 22), (511, 1022, 511 << 22), (1022, 1200, 178 << 22)]
    for z0, z1, wg, nwg, fw in pl:
        assert wg == 1024 and nwg < 2**31 and int(fw[-1]) == nwg
        for i in (0, 1, (z1 - z0) // 2, z1 - z0 - 1):
            for blk in (0, (1 << 22) - 1):
                assert find(fw, (i << 22) + blk) == i
    # in 4096-byte workgroups the same list is one launch of 1200 * 2^20
    pl = plan(8, 4, 0, sizes)
    assert [(z0, z1, nwg) for z0, z1, _, nwg, _ in pl] == [(0, 1200, 1200 << 20)]
    # one more stripe than fits 2^31 - 1 at 2^20 each
    pl = plan(8, 4, 0, [(1 << 32) - 64] * 2049)
    assert [(z0, z1) for z0, z1, *_ in pl] == [(0, 2047), (2047, 2049)]


def test_plan_refuses_bad_input():
    assert plan(8, 4, 0, [64, 0]) == INV
    assert plan(8, 4, 0, [64, 100]) == INV
    assert plan(8, 4, 0, [1 << 32]) == INV
    assert plan(12, 4, 0, [64]) == INV
    assert plan(8, 33, 0, [64]) == INV
    assert plan(8, 4, 2, [64]) == INV
    assert plan(8, 4, 0, []) == []


def test_knob_and_mirror(codecs, paths):
    L = _capi.lib()
    for v in (-1, 0, 1):
        paths("enc_list", v)
    assert L.rs_debug_set_path(b"enc_list", 2) == INV
    assert L.rs_debug_set_path(b"enc_list", -2) == INV
    assert _capi._PATH_DEFAULTS["enc_list"] == -1
    assert {"rs_encode_dev_list", "rs_verify_dev_list", "rs_debug_encode_list_plan", "rs_debug_encode_list_fits",
            "rs_debug_encode_list_own"} <= set(
        _capi.header_functions())
    one = codecs[0]
    good = torch.zeros((K + P, 128), dtype=torch.uint8)
    for fn in (one.encode_dev_list, one.verify_dev_list):
        with pytest.raises(TypeError):
            fn([good])  # not on a device
        with pytest.raises(TypeError):
            fn([torch.zeros((K + P + 1, 128), dtype=torch.uint8)])
        with pytest.raises(TypeError):
            fn([torch.zeros((2, K + P, 128), dtype=torch.uint8)])
        with pytest.raises(TypeError):
            fn([torch.zeros((K + P, 128), dtype=torch.int8)])  # one byte per element is not enough: uint8


# ---------------------------------------------------------------- the routing
# (bits, k, p) -> (the kernel a stripe alone takes, the largest size that joins the list launch; None: every size)
ROUTES = {(16, 128, 32): ("bs16-m32", 256 << 10), (16, 37, 9): ("bs16-m16", 1 << 20), (16, 192, 9): ("bs16-m16", 1 << 20),
          (16, 64, 8): ("split16-m8", 1 << 20), (16, 193, 16): ("split16-m16", 1 << 20), (16, 3, 3): ("split16-m4", 1 << 20),
          (16, 2, 1): ("reg16-m1", None), (16, 3, 2): ("reg16-m2", None), (8, 10, 4): ("reg8-m4", None),
          (8, 100, 28): ("reg8-m32", None)}


@pytest.mark.parametrize("geom", sorted(ROUTES))
def test_routing_by_the_stripes_own_kernel(geom, paths):
    """Which stripes get a launch of their own (rs_debug_encode_list_own): by the
    kernel a stripe alone takes, which rs_encode_path names, at that kernel's
    measured threshold and 64 bytes beyond; never where the register kernel is
    the only one; the knob overrides."""
    bits, k, p = geom
    path, top = ROUTES[geom]
    L = _capi.lib()
    c = rs.ReedSolomon(k, p, bits)
    try:
        assert c.encode_path == path
        own = lambda S: L.rs_debug_encode_list_own(c._h, S)  # noqa: E731
        assert own(64) == 0
        if top is None:
            assert own(1 << 30) == 0 and own((1 << 32) - 64) == 0
        else:
            assert own(top) == 0 and own(top + 64) == 1
        paths("enc_list", 0)
        assert own(64) == 1
        paths("enc_list", 1)
        assert own((1 << 32) - 64) == 0
    finally:
        c.close()


def test_routing_beyond_the_list_kernel(codecs):
    """m > 32: every stripe is a launch sequence of its own, under every knob value; no verdict for codecs the call refuses."""
    L = _capi.lib()
    for bits, k, p in ((8, 128, 128), (16, 300, 300), (16, 40, 33)):
        c = rs.ReedSolomon(k, p, bits)
        try:
            for v in (-1, 0, 1):
                _capi.set_path("enc_list", v)
                assert L.rs_debug_encode_list_own(c._h, 64) == 1
        finally:
            _capi.reset_paths()
            c.close()
    assert L.rs_debug_encode_list_own(None, 64) == -1
    assert L.rs_debug_encode_list_own(codecs[1]._h, 64) == -1
    panics = rs.New8(250, 6)
    assert L.rs_debug_encode_list_own(panics._h, 64) == -1
    panics.close()
