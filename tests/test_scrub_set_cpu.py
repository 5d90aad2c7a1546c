"""CPU tests of rs_locate_set_dev_batch's host side: the
parity-check identity the decoder rests on, re-derived here against the
oracle; the per-symbol decoder (rs_debug_locate_set) on syndromes computed with
the oracle; the cap rules; an over-capacity stripe whose "no pair explains it"
is established by brute force with the numpy oracle; and the error table of
both calls, decided before any device call.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from oracle import leopard_np, orc
from reedsolomon16_amd import _capi
from tests.scrub_set_util import explaining_sets, gf_mul, over_capacity_stripe

# the geometries the identities were first checked at, then 1024+256 and GF(2^8) 128+128
GEOMS = [(8, 10, 4), (8, 11, 5), (8, 5, 2), (8, 100, 28), (16, 37, 9), (16, 128, 32), (16, 12, 7), (16, 3, 1)]
IDENTITY_GEOMS = GEOMS + [(16, 1024, 256), (8, 128, 128)]
DECODER_GEOMS = [g for g in GEOMS if g[2] >= 4] + [(16, 1024, 256)]

FAKE = 0x10000  # a non-NULL "device pointer": every call below must return before it is used
OK, INV, NO_DATA, BAD_SIZE, PANIC = 0, 53, 4, 6, 50
S = 64


def positions(k, p):
    """Shard number -> position: data shard j at m + j, parity shard i at i."""
    m = leopard_np.ceil_pow2(p)
    return np.concatenate([m + np.arange(k), np.arange(p)]).astype(np.int64), m


def shift_point(bits, k, p):
    m = leopard_np.ceil_pow2(p)
    if p < m:
        return p
    return m + k if m + k < (1 << bits) else None


def dual_multipliers(bits, k, p):
    """u_x = the product of (x ^ y) over y in [p, m); 1 when p == m."""
    x, m = positions(k, p)
    u = np.ones(k + p, np.int64)
    for y in range(p, m):
        u = gf_mul(bits, u, x ^ y)
    return u


def encoded(bits, k, p, seed):
    rng = np.random.default_rng(seed)
    stripe = np.empty((k + p, S), np.uint8)
    stripe[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
    stripe[k:] = orc.encode(bits, k, p, stripe[:k])
    return stripe, rng


def locate_set(bits, k, p, e, max_shards=4):
    e = np.ascontiguousarray(e, np.uint32)
    count = C.c_int(-9)
    shards = np.full(max_shards, -9, np.int32)
    err = _capi.lib().rs_debug_locate_set(bits, k, p, e.ctypes.data, max_shards, C.byref(count), shards.ctypes.data)
    assert err == 0, err
    n = count.value
    assert all(s == -1 for s in shards[max(n, 0):]), "unused entries are -1"
    return n, [int(s) for s in shards[:max(n, 0)]]


@pytest.mark.parametrize("bits,k,p", IDENTITY_GEOMS)
def test_parity_check_identity(bits, k, p):
    """sum_x u_x c_x (x ^ a)^l == 0 for l < p and a in {0, the shift point}; non-zero at l = p."""
    stripe, _ = encoded(bits, k, p, bits * 911 + k * 37 + p)
    c = leopard_np.to_symbols(stripe, bits)
    x, _ = positions(k, p)
    uc = gf_mul(bits, dual_multipliers(bits, k, p)[:, None], c)
    shifts = [0] + ([shift_point(bits, k, p)] if shift_point(bits, k, p) is not None else [])
    assert (shift_point(bits, k, p) is None) == ((bits, k, p) == (8, 128, 128))
    for a in shifts:
        X = x ^ a
        if a:
            assert X.all(), "every locator is non-zero at the shift point"
        pw = np.ones(k + p, np.int64)  # 0^0 = 1
        for l in range(p + 1):
            s = np.bitwise_xor.reduce(gf_mul(bits, uc, pw[:, None]), axis=0)
            if l < p:
                assert not s.any(), f"GF(2^{bits}) {k}+{p}: check l = {l}, a = {a}"
            else:
                assert s.any(), "the code has no parity check of degree p"
            pw = gf_mul(bits, pw, X)


def injection_sets(k, p, cap, rng):
    m = leopard_np.ceil_pow2(p)
    sets = []
    for t in range(1, cap + 1):
        sets.append(sorted(int(x) for x in rng.choice(k, min(t, k), replace=False)))      # data only
        sets.append(sorted(int(k + x) for x in rng.choice(p, t, replace=False)))          # parity only
        if t >= 2 and k >= 1:
            nd = int(rng.integers(1, t))
            sets.append(sorted([int(x) for x in rng.choice(k, min(nd, k), replace=False)] +
                               [int(k + x) for x in rng.choice(p, t - nd, replace=False)]))  # mixed
    sets += [[k], [0], [k - 1], [0, k - 1], [0, k], [k - 1, k + p - 1]]
    sets.append([c * m for c in range((k + m - 1) // m)][:cap])  # one shard per encode chunk
    if cap >= 3:
        sets.append(sorted({0, k - 1, k}))
    return [sorted(set(J)) for J in sets]


@pytest.mark.parametrize("bits,k,p", DECODER_GEOMS)
def test_decoder_names_the_injected_set(bits, k, p):
    cap = min(4, p // 2)
    stripe, rng = encoded(bits, k, p, bits * 313 + k * 7 + p)
    sets = injection_sets(k, p, cap, rng)
    nsym = S // 2 if bits == 16 else S
    assert len(sets) <= nsym
    # set q is injected at symbol q: the code acts symbol by symbol
    sym = leopard_np.to_symbols(stripe, bits)
    for q, J in enumerate(sets):
        for x in J:
            sym[x, q] ^= int(rng.integers(1, 1 << bits))
    stored = leopard_np.from_symbols(sym, bits)
    e = leopard_np.to_symbols(orc.encode(bits, k, p, stored[:k]), bits) ^ sym[k:]
    for q, J in enumerate(sets):
        assert locate_set(bits, k, p, e[:, q]) == (len(J), J), f"GF(2^{bits}) {k}+{p}: set {J}"
    assert not e[:, len(sets):].any()
    assert locate_set(bits, k, p, e[:, nsym - 1]) == (0, [])
    # a smaller max_shards that still covers the set gives the same answer
    for q, J in enumerate(sets):
        if 2 <= len(J) < cap:
            assert locate_set(bits, k, p, e[:, q], len(J)) == (len(J), J)


@pytest.mark.parametrize("bits,k,p", [(16, 2, 1), (16, 3, 1), (8, 5, 2), (16, 5, 2), (16, 4, 3), (8, 128, 128)])
def test_cap_one_is_the_one_shard_route(bits, k, p):
    """p <= 3, and 128+128 where no shift point exists: cap is 1 whatever max_shards says."""
    stripe, rng = encoded(bits, k, p, bits + 31 * k + p)
    sym = leopard_np.to_symbols(stripe, bits)
    singles = sorted({0, k - 1, k, k + p - 1})
    for q, x in enumerate(singles):
        sym[x, q] ^= int(rng.integers(1, 1 << bits))
    q2 = len(singles)  # two data shards at one symbol
    if k >= 2:
        sym[0, q2] ^= 3
        sym[k - 1, q2] ^= 5
    stored = leopard_np.from_symbols(sym, bits)
    e = leopard_np.to_symbols(orc.encode(bits, k, p, stored[:k]), bits) ^ sym[k:]
    for q, x in enumerate(singles):
        want = (-1, []) if p == 1 else (1, [x])
        for ms in (1, 2, 4):
            assert locate_set(bits, k, p, e[:, q], ms) == want, f"shard {x}, max_shards {ms}"
        if p > 1 and x < k:
            shard, scale = C.c_int(-7), C.c_uint32(7)
            assert _capi.lib().rs_debug_locate(bits, k, p, int(e[0, q]), int(e[1, q]), C.byref(shard), C.byref(scale)) == 0
            assert shard.value == x
    if k >= 2:
        n4, _ = locate_set(bits, k, p, e[:, q2], 4)
        assert n4 in (-1, 1) and (n4, _) == locate_set(bits, k, p, e[:, q2], 1), "never a pair with cap 1"
    assert locate_set(bits, k, p, e[:, q2 + 1]) == (0, [])


def test_debug_locate_set_errors():
    L = _capi.lib()
    e = np.zeros(4, np.uint32)
    count, shards = C.c_int(0), np.zeros(4, np.int32)
    ok = (16, 10, 4, e.ctypes.data, 2, C.byref(count), shards.ctypes.data)
    assert L.rs_debug_locate_set(*ok) == OK and count.value == 0
    for i, v in ((0, 12), (1, 0), (2, 0), (3, None), (4, 0), (4, 5), (5, None), (6, None)):
        args = list(ok)
        args[i] = v
        assert L.rs_debug_locate_set(*args) == INV, f"argument {i} = {v}"
    assert L.rs_debug_locate_set(8, 250, 6, np.zeros(6, np.uint32).ctypes.data, 2, C.byref(count), shards.ctypes.data) == PANIC


# ---------------------------------------------------------------- over capacity
OVER_SEED = {8: 4108, 16: 4116}  # chosen so that no pair explains the stripe; checked below


@pytest.mark.parametrize("bits", [8, 16])
def test_three_random_rows_have_no_explaining_pair(bits):
    k, p = 10, 4
    good, bad, rows = over_capacity_stripe(bits, k, p, S, 3, OVER_SEED[bits])
    assert len(rows) == 3 and all((good[r] != bad[r]).any() for r in rows)
    # all 91 pairs, each by reconstructing with the pair erased and verifying the result
    assert explaining_sets(bits, k, p, bad, 2) == []
    assert explaining_sets(bits, k, p, bad, 1) == []
    # the brute force itself: with two of the rows put back, exactly the third explains the stripe ...
    part = bad.copy()
    part[rows[0]], part[rows[1]] = good[rows[0]], good[rows[1]]
    assert explaining_sets(bits, k, p, part, 1) == [(rows[2],)]
    # ... and with one put back, exactly the other two
    part = bad.copy()
    part[rows[0]] = good[rows[0]]
    assert (rows[1], rows[2]) in explaining_sets(bits, k, p, part, 2)
    # the decoder, symbol by symbol: nothing, or at most a pair, which by the above cannot explain the stripe
    e = leopard_np.to_symbols(orc.encode(bits, k, p, bad[:k]), bits) ^ leopard_np.to_symbols(bad[k:], bits)
    for q in range(e.shape[1]):
        n, J = locate_set(bits, k, p, e[:, q])
        assert n in (-1, 1, 2) if e[:, q].any() else n == 0, "never clean where e != 0, never more than cap shards"


# ---------------------------------------------------------------- the error tables
def u32(vals):
    return (C.c_uint32 * max(len(vals), 1))(*vals)


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(4, 2)
    multi = rs.New16(4, 2, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def test_locate_set_dev_batch_errors(codecs):
    one, multi = codecs
    L, h = _capi.lib(), one._h
    count = (C.c_int32 * 4)(7, 7, 7, 7)
    shards = (C.c_int32 * 16)(*([7] * 16))
    BIG = 1 << 31

    def call(c=h, base=FAKE, rs_=128, ss=6 * 128, ns=4, zs=(2, 0), nl=None, size=128, ms=2, repair=0, cn=count, sh=shards,
             nozs=False):
        arr = None if nozs else u32(zs)
        return L.rs_locate_set_dev_batch(c, base, rs_, ss, ns, arr, len(zs) if nl is None else nl, size, ms, repair, cn, sh,
                                         None)

    # RS_ERR_INVALID_ARG: the NULL arguments and max_shards, counts, the codec, the list
    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(nozs=True) == INV
    assert call(cn=None) == INV
    assert call(sh=None) == INV
    assert call(ms=0) == INV
    assert call(ms=-1) == INV
    assert call(ms=5) == INV
    assert call(ms=0, zs=()) == INV
    assert call(cn=None, nl=0) == INV
    assert call(ns=BIG) == INV
    assert call(nl=BIG) == INV
    assert call(c=multi._h) == INV
    assert call(c=multi._h, repair=1) == INV
    assert call(zs=(0, 4)) == INV
    assert call(zs=(1, 2, 1)) == INV
    # ... all before the size rules
    assert call(zs=(1, 1), size=0) == INV
    assert call(ms=9, size=0) == INV
    assert call(c=multi._h, size=100) == INV
    # the size rules, then the stride rule
    assert call(size=0) == NO_DATA
    assert call(size=100) == BAD_SIZE
    assert call(size=100, rs_=64) == BAD_SIZE
    assert call(size=192, rs_=128) == INV
    assert call(size=0, zs=(), ns=0) == NO_DATA
    # an empty list is served without a device call
    for ms in (1, 2, 3, 4):
        assert call(zs=(), ms=ms) == OK
    assert call(zs=(), repair=1) == OK
    assert list(count) == [7] * 4 and list(shards) == [7] * 16, "an error or an empty list wrote a result"


def test_scrub_set_dev_batch_errors(codecs):
    one, multi = codecs
    L, h = _capi.lib(), one._h
    count = (C.c_int32 * 4)(7, 7, 7, 7)
    shards = (C.c_int32 * 16)(*([7] * 16))
    nbad = C.c_int(9)

    def call(c=h, base=FAKE, rs_=128, ss=6 * 128, ns=4, size=128, ms=2, repair=0, cn=count, sh=shards, nb=nbad):
        return L.rs_scrub_set_dev_batch(c, base, rs_, ss, ns, size, ms, repair, cn, sh, C.byref(nb) if nb is not None else None,
                                        None)

    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(cn=None) == INV
    assert call(sh=None) == INV
    assert call(ns=0) == INV
    assert call(ns=-3) == INV
    assert call(ms=0) == INV
    assert call(ms=5) == INV
    assert call(c=multi._h) == INV
    assert call(c=multi._h, size=0) == INV
    assert call(ms=7, size=100) == INV
    assert nbad.value == 9, "an argument error touched *nbad"
    assert call(size=0) == NO_DATA
    assert nbad.value == 0
    assert call(size=100) == BAD_SIZE
    assert call(size=192, rs_=128) == INV
    assert list(count) == [7] * 4 and list(shards) == [7] * 16


def test_panic_geometry_is_refused_before_any_device_call():
    c = rs.New8(250, 6)
    L = _capi.lib()
    count, shards = (C.c_int32 * 2)(), (C.c_int32 * 8)()
    assert L.rs_locate_set_dev_batch(c._h, FAKE, S, 256 * S, 2, u32([1, 0]), 2, S, 3, 1, count, shards, None) == PANIC
    assert L.rs_locate_set_dev_batch(c._h, FAKE, S, 256 * S, 2, u32([]), 0, S, 3, 0, count, shards, None) == PANIC
    assert L.rs_scrub_set_dev_batch(c._h, FAKE, S, 256 * S, 2, S, 3, 0, count, shards, None, None) == PANIC
    c.close()


def test_python_mirror_exists():
    assert callable(rs.ReedSolomon.locate_set_dev_batch) and callable(rs.ReedSolomon.scrub_set_dev_batch)
    assert {"rs_locate_set_dev_batch", "rs_scrub_set_dev_batch", "rs_debug_locate_set"} <= set(_capi.header_functions())
    assert rs.LOCATE_SET_MAX == 4
