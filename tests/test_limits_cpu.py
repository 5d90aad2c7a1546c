"""Range limits, host side (no device): the panic verdict at the top of the
shard-count range against the oracle, the row-span predicate that admits a
strided device encode to the bit-sliced kernel (32-bit buffer offsets), and
the argument checks of the batched device calls that run before any device
work."""
import ctypes as C
import functools

import numpy as np
import pytest

import reedsolomon16_amd as rs
from oracle import orc

RS_ERR_INVALID_ARG = 53  # include/rs_mi355x.h
S_EDGE = 2048 + 192  # one full 2 KiB tile of the bit-sliced kernel plus a ragged one


def ceil_pow2(x):
    m = 1
    while m < x:
        m *= 2
    return m


def bs_fits(k, p, stride, S):
    """bitslice.hip encode_bs_fits restated: the padding rows of the last chunk
    and the lanes of the last 2 KiB tile past the row end are addressed too, and
    every one of those 32-bit offsets must stay below 2^32."""
    m = ceil_pow2(p)
    R = -(-k // m) * m
    return (R - 1) * stride + -(-S // 2048) * 2048 < 1 << 32


def last_stride(fits):
    """The largest multiple of 64 that `fits` accepts (fits is monotone)."""
    lo, hi = 1, 1 << 27  # in units of 64 bytes
    assert fits(lo * 64) and not fits(hi * 64)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid * 64) else (lo, mid)
    return lo * 64


# (k, p): the last row stride (a multiple of 64) at which S_EDGE-byte rows still
# take the bit-sliced kernel; 128 + 32 and 100 + 17 share it (m = 32, four chunks)
BS_EDGE_STRIDES = {(128, 32): 33_818_560, (100, 17): 33_818_560, (33, 12): 91_382_144}


@pytest.mark.parametrize("k,p", sorted(BS_EDGE_STRIDES))
def test_bs_fit_predicate_at_its_edge(k, p):
    L = rs.lib()
    edge = BS_EDGE_STRIDES[(k, p)]
    assert last_stride(lambda st: bs_fits(k, p, st, S_EDGE)) == edge
    assert L.rs_debug_encode_bs_fits(k, p, edge, S_EDGE) == 1
    assert L.rs_debug_encode_bs_fits(k, p, edge + 64, S_EDGE) == 0
    # other row lengths around the same strides: whole tiles, one block, a long
    # row, and strides of 4 GiB and more (no wrap of the 64-bit product)
    for S in (64, 2048, S_EDGE, 4096, 1 << 20):
        for st in (S, edge - 64, edge, edge + 64, 1 << 32, (1 << 32) + 64, 1 << 40):
            if st >= S:
                assert L.rs_debug_encode_bs_fits(k, p, st, S) == int(bs_fits(k, p, st, S)), (S, st)


@pytest.mark.parametrize("k,p", [(100, 8), (100, 33), (150, 1), (0, 16)])
def test_bs_fit_predicate_outside_the_kernel_range(k, p):
    """9 <= p <= 32 and k >= 1 only: every other geometry is refused at any stride."""
    assert rs.lib().rs_debug_encode_bs_fits(k, p, 4096, 2048) == 0


P_SWEEP = [1, 2, 3, 31, 32, 33, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 40000, 65535]


def panic_cases(bits):
    order = 1 << bits
    out = []
    for p in P_SWEEP:
        m = ceil_pow2(p)
        for k in sorted({order - p, order - m, order - m - 1, order - m + 1, 1}):
            if k >= 1 and k + p <= order:
                out.append((bits, k, p))
    return out


PANIC_CASES = panic_cases(16) + panic_cases(8)


@functools.lru_cache(maxsize=None)
def oracle_verdict(bits, k, p):
    """The oracle's encode return code for one 64-byte block per shard."""
    return orc.Oracle(bits, k, p).encode(list(np.zeros((k + p, 64), np.uint8)))


@pytest.mark.parametrize("bits,k,p", PANIC_CASES)
def test_panic_verdict_equals_oracle(bits, k, p):
    """The reference panics (index out of range in its skew tables) for some
    geometries at the top of the range; the oracle models that as code 50 and
    the engine decides it when the codec is made, without a device."""
    eo = oracle_verdict(bits, k, p)
    assert eo in (0, 50)
    c = rs.ReedSolomon(k, p, bits)
    assert (c.encode_path == "panic") == (eo == 50), (c.encode_path, eo)
    if eo == 50:
        with pytest.raises(rs.ErrPanic):
            c.encode(list(np.zeros((k + p, 64), np.uint8)))


@pytest.mark.parametrize("bits", [16, 8])
def test_panic_sweep_holds_both_verdicts(bits):
    """The sweep is a comparison of verdicts only while the oracle gives both
    in each field (today 17 panics of 62 cases in GF(2^16), 4 of 22 in GF(2^8))."""
    got = {oracle_verdict(b, k, p) for b, k, p in PANIC_CASES if b == bits}
    assert got == {0, 50}


@pytest.mark.parametrize("bits,k,p", [(8, 10, 4), (16, 128, 32), (16, 100, 40)])
def test_batch_calls_reject_row_stride_below_shard_size(bits, k, p):
    """rs_encode_dev_batch / rs_verify_dev_batch: rows that overlap
    (row_stride < S) are an argument error, found before any device call (the
    base pointer is never dereferenced), as rs_reconstruct_dev_batch has it."""
    c = rs.ReedSolomon(k, p, bits)
    L, S, base = rs.lib(), 256, 1 << 20
    ok = C.c_int(7)
    for stride in (0, 64, S - 64):
        assert L.rs_encode_dev_batch(c._h, base, stride, (k + p) * S, 2, S, None) == RS_ERR_INVALID_ARG
        assert L.rs_verify_dev_batch(c._h, base, stride, (k + p) * S, 2, S, C.byref(ok), None) == RS_ERR_INVALID_ARG
        assert ok.value == 0
        ok.value = 7
    pr = (C.c_uint8 * (k + p))(*([0] + [1] * (k + p - 1)))
    assert L.rs_reconstruct_dev_batch(c._h, base, S - 64, (k + p) * S, 2, pr, S, 1, None) == RS_ERR_INVALID_ARG


# ---- the layouts of tests/test_gpu_limits.py
from tests import limits_cases as lc  # noqa: E402


def test_gpu_limit_cases_are_what_they_claim():
    """tests/test_gpu_limits.py takes its shapes and layouts from
    limits_cases.py: every layout must fit the one 6 GiB buffer, the far
    geometries must be far, and each encode case must name the kernel its codec
    takes (the bit-sliced one only while its row predicate holds)."""
    assert lc.S_EDGE == S_EDGE
    shapes = set(lc.REC_SHAPES + lc.ROWS_SHAPES + lc.UPDATE_SHAPES + lc.SCRUB_SHAPES + [lc.CHECKED_SHAPE] +
                 [c[:3] for c in lc.FAR_STRIPE_ENCODES])
    assert {c[:3] for c in lc.REC_CASES} == set(lc.REC_SHAPES)
    for bits, k, p in shapes:
        n = k + p
        base, rstride, sstride = lc.geometry("far_rows", n)
        assert rstride % 64 == 0 and base + (n - 1) * rstride + 4 * lc.MIB + S_EDGE + lc.GUARD <= lc.BUF_BYTES
        assert (n - 1) * rstride + S_EDGE >= 1 << 32  # the stripe's rows span 4 GiB
        # and so do its data rows alone, wherever k of k + p rows in 6 GiB can
        assert (k - 1) * rstride + S_EDGE >= 1 << 32 or (k - 1) * lc.BUF_BYTES < (n - 1) << 32, (bits, k, p)
        base, rstride, sstride = lc.geometry("far_stripes", n)
        assert rstride == lc.NEAR_ROW and sstride >= 1 << 32
        assert base + sstride + 16 * lc.MIB + n * rstride + lc.GUARD <= lc.BUF_BYTES
    for bits, k, p, path in lc.FAR_STRIPE_ENCODES + lc.GRID_ENCODES:
        assert rs.ReedSolomon(k, p, bits).encode_path == path, (bits, k, p)
    assert rs.lib().rs_debug_encode_bs_fits(128, 32, lc.NEAR_ROW, S_EDGE) == 1
    assert [c[3].split("-")[0].rstrip("168") for c in lc.GRID_ENCODES] == ["reg", "split", "lds"]  # the unsliced launchers
    assert lc.GRID_STRIPES > 65_535 and (1 << 32) + lc.GUARD + lc.GRID_STRIPES * 37 * lc.GRID_S + lc.GUARD <= lc.BUF_BYTES
