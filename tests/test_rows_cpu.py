"""CPU tests of the selective reconstruct's host side: the decode coefficients
(rs_debug_decode_coefficients, csrc/gf_host.cpp decode_coefficients) against
the oracle's reconstruct of unit stripes, the linear model the direct kernel
evaluates, and the error rules of rs_reconstruct_rows_dev /
rs_reconstruct_rows_dev_batch / rs_reconstruct_rows, which are all decided
before any device call.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from oracle import leopard_np, orc
from reedsolomon16_amd import _capi

GEOMS16 = [(128, 32), (37, 9), (3, 7), (2, 1), (1, 1), (300, 300)]
GEOMS8 = [(10, 4), (100, 28), (128, 128)]
GEOMS = [(16, k, p) for k, p in GEOMS16] + [(8, k, p) for k, p in GEOMS8]
PATTERNS = ["one", "p", "parity"]


def pattern(kind, bits, k, p):
    """present flags: one data row erased; p rows erased (a data / parity mix);
    parity rows only (up to three)."""
    rng = np.random.default_rng(bits * 1000003 + k * 1009 + p * 13 + len(kind))
    present = np.ones(k + p, bool)
    if kind == "one":
        present[int(rng.integers(0, k))] = False
    elif kind == "p":
        present[rng.choice(k + p, p, replace=False)] = False
    else:
        present[k + rng.choice(p, min(p, 3), replace=False)] = False
    return present


def some(rows, count=3):
    """First, last and middle of a list of rows (all of them when it is short)."""
    rows = [int(r) for r in rows]
    return sorted({rows[0], rows[-1], rows[len(rows) // 2]}) if len(rows) > count else rows


def coefficients(bits, k, p, present, row):
    out = np.zeros(k + p, np.uint32)
    pr = (C.c_uint8 * (k + p))(*[1 if x else 0 for x in present])
    e = _capi.lib().rs_debug_decode_coefficients(bits, k, p, pr, row, out.ctypes.data)
    assert e == 0, e
    return out.astype(np.int64)


def oracle_rows(bits, k, p, shards, present):
    """The oracle's Reconstruct of the rows marked present: {missing index: bytes}."""
    lst = [np.ascontiguousarray(shards[i]) if present[i] else None for i in range(k + p)]
    e, out = orc.Oracle(bits, k, p).reconstruct(lst, recover_all=True)
    assert e == 0, e
    return {i: out[i] for i in range(k + p) if not present[i]}


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("bits,k,p", GEOMS)
def test_coefficients_match_oracle_unit_stripes(bits, k, p, kind):
    """Symbol 1 in one present row, zeros elsewhere: the oracle's rebuilt symbol
    in row r is D[r][that row].  Columns are independent, so one 64-byte stripe
    carries a unit stripe per symbol column, each for another present row."""
    S = 64
    nsym = S // 2 if bits == 16 else S
    present = pattern(kind, bits, k, p)
    rows_present = np.flatnonzero(present)
    wanted = some(np.flatnonzero(~present))
    got = {r: coefficients(bits, k, p, present, r) for r in wanted}
    for r in wanted:
        assert not got[r][~present].any(), "a missing row has a coefficient"
    for b in range(0, len(rows_present), nsym):
        batch = rows_present[b:b + nsym]
        sym = np.zeros((k + p, nsym), np.int64)
        sym[batch, np.arange(len(batch))] = 1
        out = oracle_rows(bits, k, p, leopard_np.from_symbols(sym, bits), present)
        for r in wanted:
            want = leopard_np.to_symbols(out[r][None], bits)[0][:len(batch)]
            assert np.array_equal(got[r][batch], want), f"{bits} {k}+{p} {kind} row {r} batch {b}"


@pytest.mark.parametrize("bits,k,p,kind", [
    (16, 128, 32, "p"), (16, 37, 9, "p"), (16, 3, 7, "p"), (16, 128, 32, "one"),
    (8, 10, 4, "p"), (8, 100, 28, "p"), (8, 128, 128, "parity"),
])
def test_linear_model_on_an_inconsistent_stripe(bits, k, p, kind):
    """XOR over present j of D[r][j] * row_j == the oracle's row r, for rows
    that are no codeword (random bytes in every present row)."""
    S = 128
    F = leopard_np.field(bits)
    present = pattern(kind, bits, k, p)
    rng = np.random.default_rng(bits * 7 + k * 31 + p)
    shards = rng.integers(0, 256, (k + p, S), dtype=np.uint8)
    out = oracle_rows(bits, k, p, shards, present)
    sym = leopard_np.to_symbols(shards, bits)
    for r in some(np.flatnonzero(~present)):
        co = coefficients(bits, k, p, present, r)
        acc = np.zeros(sym.shape[1], np.int64)
        for j in np.flatnonzero(present):
            if co[j]:  # a zero coefficient contributes nothing; its log is not a log
                acc ^= F.mul_log(sym[j], int(F._log[co[j]]))
        assert np.array_equal(acc, leopard_np.to_symbols(out[r][None], bits)[0]), f"row {r}"


def test_decode_coefficients_errors():
    L = _capi.lib()
    out = np.zeros(64, np.uint32)
    o = out.ctypes.data
    pr = (C.c_uint8 * 6)(1, 1, 0, 1, 1, 1)
    INV, PANIC = 53, 50
    assert L.rs_debug_decode_coefficients(12, 4, 2, pr, 2, o) == INV
    assert L.rs_debug_decode_coefficients(16, 4, 2, None, 2, o) == INV
    assert L.rs_debug_decode_coefficients(16, 4, 2, pr, 2, None) == INV
    assert L.rs_debug_decode_coefficients(16, 0, 2, pr, 0, o) == INV
    assert L.rs_debug_decode_coefficients(16, 4, 0, pr, 0, o) == INV
    assert L.rs_debug_decode_coefficients(16, 4, 2, pr, -1, o) == INV
    assert L.rs_debug_decode_coefficients(16, 4, 2, pr, 6, o) == INV
    assert L.rs_debug_decode_coefficients(16, 4, 2, pr, 2, o) == 0
    # GF(2^8) with m + k > 256: the reference's reconstruct panics
    big = (C.c_uint8 * 264)(*([1] * 264))
    assert L.rs_debug_decode_coefficients(8, 250, 14, big, 0, np.zeros(264, np.uint32).ctypes.data) == PANIC


# ---------------------------------------------------------------- error rules (no device call)
FAKE = 0x10000  # a non-NULL "device pointer": every call below must return before it is used
INV, TOO_FEW, NO_DATA, SHARD_SIZE, BAD_SIZE = 53, 3, 4, 5, 6
K, P, N = 4, 2, 6


def ptr_array(vals):
    return (C.c_void_p * len(vals))(*vals)


def flags(vals):
    return (C.c_uint8 * len(vals))(*vals)


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(K, P)
    multi = rs.New16(K, P, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def test_rows_dev_errors(codecs):
    one, multi = codecs
    L, h = _capi.lib(), one._h
    rows = ptr_array([FAKE] * N)
    pr = flags([1, 1, 0, 1, 1, 0])
    req = flags([0, 0, 1, 0, 0, 0])
    S = 128
    f = L.rs_reconstruct_rows_dev
    assert f(None, rows, pr, req, S, None) == INV
    assert f(h, None, pr, req, S, None) == INV
    assert f(h, rows, None, req, S, None) == INV
    assert f(h, rows, pr, None, S, None) == INV
    assert f(multi._h, rows, pr, req, S, None) == INV
    assert f(h, rows, flags([0] * N), req, S, None) == NO_DATA
    assert f(h, rows, pr, req, 0, None) == NO_DATA
    # nothing to rebuild: RS_OK before anything else is looked at, nothing launched
    assert f(h, rows, pr, flags([0] * N), S, None) == 0
    assert f(h, rows, pr, flags([1, 1, 0, 1, 1, 0]), S, None) == 0      # flags only on present rows
    assert f(h, rows, flags([1] * N), flags([1] * N), 100, None) == 0   # nothing missing
    assert f(h, ptr_array([None] * N), flags([1, 0, 0, 0, 0, 0]), flags([1, 0, 0, 0, 0, 0]), 100, None) == 0
    # too few present is decided before the size
    assert f(h, rows, flags([1, 1, 0, 1, 0, 0]), req, 100, None) == TOO_FEW
    assert f(h, rows, pr, req, 100, None) == BAD_SIZE
    # NULL row pointers: a present row, the wanted row (an unwanted missing row may be NULL)
    assert f(h, ptr_array([FAKE, None, FAKE, FAKE, FAKE, None]), pr, req, S, None) == INV
    assert f(h, ptr_array([FAKE, FAKE, None, FAKE, FAKE, None]), pr, req, S, None) == INV


def test_rows_dev_batch_errors(codecs):
    one, multi = codecs
    L, h = _capi.lib(), one._h
    pr = flags([1, 1, 0, 1, 1, 0])
    req = flags([0, 0, 1, 0, 0, 1])
    S = 128

    def call(c=h, base=FAKE, rs_=S, ss=N * S, ns=2, present=pr, required=req, size=S):
        return L.rs_reconstruct_rows_dev_batch(c, base, rs_, ss, ns, present, required, size, None)

    assert call(c=None) == INV
    assert call(base=None) == INV
    assert call(present=None) == INV
    assert call(required=None) == INV
    assert call(ns=0) == INV
    assert call(ns=1 << 31) == INV
    assert call(c=multi._h) == INV
    assert call(present=flags([0] * N)) == NO_DATA
    assert call(size=0) == NO_DATA
    assert call(required=flags([1, 1, 0, 1, 1, 0])) == 0
    assert call(required=flags([0] * N), rs_=0) == 0  # nothing to do comes before the strides
    assert call(present=flags([1, 0, 0, 1, 1, 0])) == TOO_FEW
    assert call(size=100) == BAD_SIZE
    assert call(rs_=S - 64) == INV
    assert call(ss=N * S - 64) == INV
    assert call(rs_=2 * S, ss=N * S) == INV


@pytest.mark.parametrize("which", [0, 1], ids=["single", "multi"])
def test_rows_host_errors(codecs, which):
    c = codecs[which]
    L, h = _capi.lib(), c._h
    S = 128
    bufs = [np.zeros(S, np.uint8) for _ in range(N)]
    ptrs = ptr_array([b.ctypes.data for b in bufs])

    def lens(present, size=S):
        return (C.c_size_t * N)(*[size if x else 0 for x in present])

    pr = [1, 1, 0, 1, 1, 0]
    req = flags([0, 0, 1, 0, 0, 0])
    f = L.rs_reconstruct_rows
    assert f(None, ptrs, lens(pr), N, req) == INV
    assert f(h, None, lens(pr), N, req) == INV
    assert f(h, ptrs, None, N, req) == INV
    assert f(h, ptrs, lens(pr), N, None) == INV
    assert f(h, ptrs, lens(pr), N - 1, req) == TOO_FEW
    assert f(h, ptrs, lens([0] * N), N, req) == NO_DATA
    ln = lens(pr)
    ln[1] = 64
    assert f(h, ptrs, ln, N, req) == SHARD_SIZE
    ln = lens(pr)
    assert f(h, ptrs, ln, N, flags([1, 1, 0, 1, 1, 0])) == 0  # flags only on present rows: nothing to do
    assert list(ln) == [S, S, 0, S, S, 0]
    assert f(h, ptrs, lens([1, 1, 0, 1, 0, 0]), N, req) == TOO_FEW
    assert f(h, ptrs, lens(pr, 96), N, req) == BAD_SIZE
    ln = lens(pr)
    assert f(h, ptr_array([b.ctypes.data for b in bufs[:2]] + [None] + [b.ctypes.data for b in bufs[3:]]), ln, N, req) == INV
    assert list(ln) == [S, S, 0, S, S, 0]


def test_rows_direct_knob(paths):
    L = _capi.lib()
    for v in (-1, 0, 1):
        paths("rows_direct", v)
    assert L.rs_debug_set_path(b"rows_direct", 2) == INV
    assert L.rs_debug_set_path(b"rows_direct", -2) == INV


def test_reconstruct_some_is_still_the_reference_mirror():
    """reconstruct_some keeps reading only len(required); the new names are separate."""
    for name in ("reconstruct_rows", "reconstruct_rows_dev", "reconstruct_rows_dev_batch"):
        assert callable(getattr(rs.ReedSolomon, name))
