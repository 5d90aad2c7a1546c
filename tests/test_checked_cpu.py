"""CPU tests of rs_reconstruct_checked_dev_batch_patterns' host side (DESIGN.md
4.18), each identity re-derived against the oracle: the check matrix's columns
(rs_debug_check_column), the power-sum identity of the filled stripe over the
corrupt survivors and the rebuilt rows, the errors-and-erasures decoder
(rs_debug_locate_set_present) on oracle syndromes, a brute force at 10+4 with
one row missing, and the call's error table, decided before any device call.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from oracle import leopard_np
from reedsolomon16_amd import _capi
from tests.checked_util import codeword, explaining_survivor_sets, fill, syndrome
from tests.scrub_set_util import gf_mul
from tests.test_scrub_set_cpu import dual_multipliers, locate_set, positions, shift_point

FAKE = 0x10000  # a non-NULL "device pointer": every call below must return before it is used
OK, INV, NO_DATA, TOO_FEW, BAD_SIZE, PANIC = 0, 53, 4, 3, 6, 50
S = 64

# geometry and the numbers of missing rows it is checked at
COLUMN_CASES = [(16, 12, 7, 1), (16, 12, 7, 3), (16, 12, 7, 5), (16, 10, 4, 1), (16, 10, 4, 2), (16, 37, 9, 4),
                (16, 128, 32, 1), (16, 128, 32, 30), (8, 10, 4, 2), (8, 100, 28, 9)]


def missing_rows(k, p, e, rng):
    """e missing rows with parity row 1 among them; data shards 0 and k - 1 and
    parity shards 0 and 2 (next to the missing one) stay."""
    keep = {0, k - 1, k, k + 2, k + 1}
    rest = [i for i in range(k + p) if i not in keep]
    return sorted([k + 1] + [int(x) for x in rng.choice(rest, e - 1, replace=False)])


def present_flags(k, p, missing):
    pr = np.ones(k + p, np.uint8)
    pr[list(missing)] = 0
    return pr


def check_column(bits, k, p, present, t):
    out = np.full(p, 0xDEAD, np.uint32)
    err = _capi.lib().rs_debug_check_column(bits, k, p, present.ctypes.data_as(C.POINTER(C.c_uint8)), t, out.ctypes.data)
    assert err == OK, err
    return out.astype(np.int64)


def locate_present(bits, k, p, present, e, cap=4):
    e = np.ascontiguousarray(e, np.uint32)
    count = C.c_int(-9)
    shards = np.full(max(cap, 1), -9, np.int32)
    err = _capi.lib().rs_debug_locate_set_present(bits, k, p, present.ctypes.data_as(C.POINTER(C.c_uint8)), e.ctypes.data,
                                                  cap, C.byref(count), shards.ctypes.data)
    assert err == OK, err
    n = count.value
    assert all(s == -1 for s in shards[max(n, 0):]), "unused entries are -1"
    return n, [int(s) for s in shards[:max(n, 0)]]


@pytest.mark.parametrize("bits,k,p,e", COLUMN_CASES)
def test_effective_columns(bits, k, p, e):
    """A difference D in survivor t moves syndrome row i of the filled stripe by H[i][t] * D."""
    good, rng = codeword(bits, k, p, S, bits * 101 + k * 13 + p * 7 + e)
    E = missing_rows(k, p, e, rng)
    pr = present_flags(k, p, E)
    assert not syndrome(bits, k, p, fill(bits, k, p, good, E)).any(), "consistent survivors: the fill is the codeword"
    for t in (0, k - 1, k, k + 2):
        bad = good.copy()
        bad[t] ^= rng.integers(1, 256, S, dtype=np.uint8)
        D = leopard_np.to_symbols(bad[t:t + 1], bits)[0] ^ leopard_np.to_symbols(good[t:t + 1], bits)[0]
        bad[E] = rng.integers(0, 256, (len(E), S), dtype=np.uint8)  # a missing row's content is never read
        got = syndrome(bits, k, p, fill(bits, k, p, bad, E))
        H = check_column(bits, k, p, pr, t)
        assert np.array_equal(got, gf_mul(bits, H[:, None], D[None, :])), f"GF(2^{bits}) {k}+{p}, E = {E}, t = {t}"
        assert H.any()


@pytest.mark.parametrize("bits,k,p,e", [(16, 12, 7, 3), (16, 37, 9, 4), (8, 10, 4, 1), (8, 100, 28, 9), (16, 128, 32, 30)])
def test_syndrome_identity(bits, k, p, e):
    """S_l of the filled stripe == sum over T and E of u_x * d_x * X_x^l for every l < p."""
    good, rng = codeword(bits, k, p, S, bits * 211 + k + p * 5 + e)
    E = missing_rows(k, p, e, rng)
    bad = good.copy()
    T = [0, k]
    for t in T:
        bad[t] ^= rng.integers(1, 256, S, dtype=np.uint8)
    f = fill(bits, k, p, bad, E)
    d = leopard_np.to_symbols(f, bits) ^ leopard_np.to_symbols(good, bits)
    assert not d[[i for i in range(k + p) if i not in E + T]].any()
    assert all(d[x].any() for x in E), "a corrupt survivor reaches every rebuilt row"
    x, _ = positions(k, p)
    a = shift_point(bits, k, p)
    X = x ^ a
    u = dual_multipliers(bits, k, p)
    ei = syndrome(bits, k, p, f)
    pw = np.ones(k + p, np.int64)
    for l in range(p):
        lhs = np.bitwise_xor.reduce(gf_mul(bits, gf_mul(bits, u[k:], pw[k:])[:, None], ei), axis=0)
        rhs = np.bitwise_xor.reduce(gf_mul(bits, gf_mul(bits, u, pw)[:, None], d), axis=0)
        assert np.array_equal(lhs, rhs), f"l = {l}"
        pw = gf_mul(bits, pw, X)


def survivor_sets(k, p, E, cap, rng):
    alive_d = [i for i in range(k) if i not in E]
    alive_p = [i for i in range(k, k + p) if i not in E]
    sets = []
    for t in range(1, cap + 1):
        if len(alive_d) >= t:
            sets.append([int(x) for x in rng.choice(alive_d, t, replace=False)])
        if len(alive_p) >= t:
            sets.append([int(x) for x in rng.choice(alive_p, t, replace=False)])
        if t >= 2 and alive_d and len(alive_p) >= t - 1:
            sets.append([int(rng.choice(alive_d))] + [int(x) for x in rng.choice(alive_p, t - 1, replace=False)])
    sets += [[alive_d[0]], [alive_d[-1]], [alive_p[0]], [alive_p[-1]]]
    return [sorted(set(J)) for J in sets]


def patterns_for(k, p, e, rng):
    """Missing data only, missing parity only, and a pattern without parity shard 0."""
    out = []
    if e == 0:
        return [[]]
    if e <= k - 2:
        out.append(sorted(int(x) for x in rng.choice(k, e, replace=False)))
    if e <= p - 1:
        out.append(sorted(int(k + x) for x in rng.choice(np.arange(1, p), e, replace=False)))
    rest = [i for i in range(k + p) if i != k]
    out.append(sorted([k] + [int(x) for x in rng.choice(rest, e - 1, replace=False)]))
    return out


DECODER_CASES = [(16, 12, 7, None), (16, 10, 4, None), (8, 10, 4, None), (16, 37, 9, None), (8, 100, 28, (0, 1, 9, 20, 26)),
                 (16, 128, 32, (1, 24, 30))]


@pytest.mark.parametrize("bits,k,p,es", DECODER_CASES)
def test_decoder_names_the_corrupt_survivors(bits, k, p, es):
    for e in (es if es is not None else range(p - 1)):
        cap = min(4, (p - e) // 2)
        good, rng = codeword(bits, k, p, S, bits * 17 + k * 3 + p + 1000 * e)
        for E in patterns_for(k, p, e, rng):
            pr = present_flags(k, p, E)
            sets = survivor_sets(k, p, E, cap, rng) if cap else []
            over = None  # cap + 1 corrupt survivors, still within the distance
            if 2 * (cap + 1) + e <= p:
                alive = [i for i in range(k + p) if i not in E]
                over = sorted(int(x) for x in rng.choice(alive, cap + 1, replace=False))
            nsym = S // 2 if bits == 16 else S
            assert len(sets) + 2 <= nsym
            sym = leopard_np.to_symbols(good, bits)
            for q, J in enumerate(sets):  # set q is injected at symbol q: the code acts symbol by symbol
                for x in J:
                    sym[x, q] ^= int(rng.integers(1, 1 << bits))
            q_over = len(sets)
            for x in over or []:
                sym[x, q_over] ^= int(rng.integers(1, 1 << bits))
            bad = leopard_np.from_symbols(sym, bits)
            ei = syndrome(bits, k, p, fill(bits, k, p, bad, E, numpy_oracle=False))
            for q, J in enumerate(sets):
                assert locate_present(bits, k, p, pr, ei[:, q], 4) == (len(J), J), f"GF(2^{bits}) {k}+{p} E = {E}: set {J}"
                if e == 0:
                    assert locate_present(bits, k, p, pr, ei[:, q], 4) == locate_set(bits, k, p, ei[:, q], 4)
                if len(J) >= 2:
                    assert locate_present(bits, k, p, pr, ei[:, q], len(J)) == (len(J), J)
                    if e:
                        assert locate_present(bits, k, p, pr, ei[:, q], len(J) - 1)[0] == -1
            if over is not None:
                assert ei[:, q_over].any()
                if e:  # (nothing missing is the set locate's decoder, which reads 2 * cap syndromes only)
                    assert locate_present(bits, k, p, pr, ei[:, q_over], 4)[0] == -1, f"E = {E}: {over} is past cap {cap}"
                if e == 0 and cap >= 1:
                    assert locate_present(bits, k, p, pr, ei[:, q_over], 4) == locate_set(bits, k, p, ei[:, q_over], 4)
            assert not ei[:, q_over + 1:].any()
            assert locate_present(bits, k, p, pr, ei[:, nsym - 1], 4) == (0, [])
            assert locate_present(bits, k, p, pr, ei[:, nsym - 1], 0) == (0, [])
            if sets:
                assert locate_present(bits, k, p, pr, ei[:, 0], 0)[0] == -1, "cap 0 locates nothing"


@pytest.mark.parametrize("bits,k,p", [(16, 12, 7), (8, 10, 4), (16, 2, 1), (16, 5, 2)])
def test_no_redundancy_left_locates_nothing(bits, k, p):
    """p - e <= 1: any inconsistency is -1."""
    for e in (p - 1, p):
        good, rng = codeword(bits, k, p, S, bits + k + p + e)
        E = sorted(int(x) for x in rng.choice(np.arange(1, k + p), e, replace=False)) if e else []
        if not E:
            continue
        pr = present_flags(k, p, E)
        bad = good.copy()
        bad[0, :4] ^= 0x5A
        ei = syndrome(bits, k, p, fill(bits, k, p, bad, E, numpy_oracle=False))
        if e == p:
            assert not ei.any(), "with p rows missing every survivor set is consistent"
        else:
            assert ei[:, 0].any()
            assert locate_present(bits, k, p, pr, ei[:, 0], 4)[0] == -1


def test_no_shift_point_locates_nothing():
    bits, k, p = 8, 128, 128
    good, rng = codeword(bits, k, p, S, 77)
    E = [5]
    bad = good.copy()
    bad[9, 0] ^= 1
    ei = syndrome(bits, k, p, fill(bits, k, p, bad, E, numpy_oracle=False))
    assert ei[:, 0].any()
    assert locate_present(bits, k, p, present_flags(k, p, E), ei[:, 0], 4)[0] == -1
    assert locate_present(bits, k, p, present_flags(k, p, E), ei[:, 1], 4) == (0, [])


@pytest.mark.parametrize("bits", [8, 16])
def test_brute_force_one_row_missing(bits):
    """10+4 with one row missing (cap_z = 1): the located survivor is the only
    single survivor whose removal makes the rest consistent."""
    k, p = 10, 4
    for miss, t in ((3, 7), (k + 1, 2), (k, k + 3), (0, k)):
        good, rng = codeword(bits, k, p, S, bits * 5 + miss * 31 + t)
        bad = good.copy()
        bad[t] = rng.integers(0, 256, S, dtype=np.uint8)
        bad[t, 0] = good[t, 0] ^ 0x5A
        bad[t, 32] = good[t, 32] ^ 0x11  # (GF(2^16): symbol 0 differs in both bytes)
        bad[miss] = 0
        assert explaining_survivor_sets(bits, k, p, bad, [miss], 0) == []
        assert explaining_survivor_sets(bits, k, p, bad, [miss], 1) == [(t,)]
        pr = present_flags(k, p, [miss])
        ei = syndrome(bits, k, p, fill(bits, k, p, bad, [miss]))
        for q in range(ei.shape[1]):
            want = (1, [t]) if ei[:, q].any() else (0, [])
            assert locate_present(bits, k, p, pr, ei[:, q], 4) == want
        assert ei[:, 0].any()
        # two corrupt survivors are past cap_z = 1: no single survivor explains them
        bad[(t + 1) % k if t < k else k + 2] ^= 0x21
        assert explaining_survivor_sets(bits, k, p, bad, [miss], 1) == []


def test_debug_errors():
    L = _capi.lib()
    pr = np.ones(14, np.uint8)
    pr[3] = 0
    prp = pr.ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.zeros(4, np.uint32)
    assert L.rs_debug_check_column(16, 10, 4, prp, 0, out.ctypes.data) == OK
    assert L.rs_debug_check_column(16, 10, 4, prp, 3, out.ctypes.data) == INV, "a missing row has no column"
    assert L.rs_debug_check_column(16, 10, 4, prp, 14, out.ctypes.data) == INV
    assert L.rs_debug_check_column(16, 10, 4, prp, -1, out.ctypes.data) == INV
    assert L.rs_debug_check_column(12, 10, 4, prp, 0, out.ctypes.data) == INV
    assert L.rs_debug_check_column(16, 10, 4, None, 0, out.ctypes.data) == INV
    assert L.rs_debug_check_column(16, 10, 4, prp, 0, None) == INV
    e = np.zeros(4, np.uint32)
    count, shards = C.c_int(0), np.zeros(4, np.int32)
    assert L.rs_debug_locate_set_present(16, 10, 4, prp, e.ctypes.data, 5, C.byref(count), shards.ctypes.data) == INV
    assert L.rs_debug_locate_set_present(16, 10, 4, prp, e.ctypes.data, -1, C.byref(count), shards.ctypes.data) == INV
    assert L.rs_debug_locate_set_present(16, 10, 4, None, e.ctypes.data, 1, C.byref(count), shards.ctypes.data) == INV
    assert L.rs_debug_locate_set_present(16, 10, 4, prp, None, 1, C.byref(count), shards.ctypes.data) == INV
    assert L.rs_debug_locate_set_present(16, 10, 4, prp, e.ctypes.data, 1, None, shards.ctypes.data) == INV
    assert L.rs_debug_locate_set_present(16, 10, 4, prp, e.ctypes.data, 1, C.byref(count), None) == INV
    assert L.rs_debug_locate_set_present(16, 10, 4, prp, e.ctypes.data, 1, C.byref(count), shards.ctypes.data) == OK
    assert count.value == 0


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


def test_checked_errors(codecs):
    one, multi = codecs
    L, h = _capi.lib(), one._h
    count = (C.c_int32 * 4)(7, 7, 7, 7)
    shards = (C.c_int32 * 16)(*([7] * 16))
    nbad = C.c_int(9)
    BIG = 1 << 31
    table = np.array([[1, 1, 1, 1, 1, 0], [0, 1, 1, 1, 1, 1]], np.uint8)

    def call(c=h, base=FAKE, rs_=128, ss=6 * 128, ns=4, tab=table, npat=None, of=(0, 1, 1, 0), size=128, ms=2, repair=0,
             cn=count, sh=shards, nb=nbad, notab=False, noof=False):
        t = None if notab else np.ascontiguousarray(tab).ctypes.data_as(C.POINTER(C.c_uint8))
        return L.rs_reconstruct_checked_dev_batch_patterns(
            c, base, rs_, ss, ns, t, len(tab) if npat is None else npat, None if noof else u32(of), size, ms, repair, cn, sh,
            C.byref(nb) if nb is not None else None, None)

    # RS_ERR_INVALID_ARG: the NULL arguments, count and shards among them, the counts, the codec
    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(notab=True) == INV
    assert call(noof=True) == INV
    assert call(cn=None) == INV
    assert call(sh=None) == INV
    assert call(ns=BIG) == INV
    assert call(c=multi._h) == INV
    assert call(c=multi._h, repair=1) == INV
    assert call(npat=0) == INV
    assert call(npat=65537) == INV
    assert nbad.value == 9, "an argument error touched *nbad"
    # the table, in rs_reconstruct_dev_batch_patterns' order
    assert call(of=(0, 2, 0, 0)) == INV
    assert nbad.value == 0
    assert call(of=(0, 2, 0, 0), size=0) == INV
    assert call(size=0) == NO_DATA
    none = np.array([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]], np.uint8)
    assert call(tab=none) == NO_DATA
    few = np.array([[1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1]], np.uint8)
    assert call(tab=few) == TOO_FEW
    assert call(tab=few, size=100) == TOO_FEW
    assert call(size=100) == BAD_SIZE
    assert call(size=192, rs_=128) == INV
    assert call(ss=5 * 128) == INV
    # max_shards comes after the table
    assert call(ms=-1) == INV
    assert call(ms=5) == INV
    assert call(ms=5, size=0) == NO_DATA
    assert call(ms=5, tab=few) == TOO_FEW
    assert call(ms=9, size=100) == BAD_SIZE
    assert call(cn=None, size=0) == INV
    assert list(count) == [7] * 4 and list(shards) == [7] * 16, "an error wrote a result"
    # no stripe: served without a device call, for every max_shards
    for ms in (0, 1, 4):
        assert call(ns=0, of=(), ms=ms) == OK
    assert list(count) == [7] * 4


def test_panic_geometry_is_refused_before_any_device_call():
    c = rs.New8(250, 6)
    L = _capi.lib()
    count, shards = (C.c_int32 * 2)(), (C.c_int32 * 8)()
    table = np.ones((1, 256), np.uint8)
    table[0, 3] = 0
    assert L.rs_reconstruct_checked_dev_batch_patterns(
        c._h, FAKE, S, 256 * S, 2, table.ctypes.data_as(C.POINTER(C.c_uint8)), 1, u32([0, 0]), S, 2, 0, count, shards, None,
        None) == PANIC
    c.close()


def test_python_mirror_exists():
    assert callable(rs.ReedSolomon.reconstruct_checked_dev_batch_patterns)
    assert {"rs_reconstruct_checked_dev_batch_patterns", "rs_debug_check_column", "rs_debug_locate_set_present",
            "rs_debug_checked_stats"} <= set(_capi.header_functions())
