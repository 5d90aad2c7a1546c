"""GPU tests of the degraded read of a list of stripes of different sizes
(rs_reconstruct_rows_dev_list; stream_kernels.hip k_decode_rows_list) against the
oracle: after a call the whole buffer that holds the stripes must be, bit for
bit, the expected image -- a fresh oracle's Reconstruct per stripe in the rows
that are missing and required, and every other byte as it was: present rows,
missing rows not asked for, stripes with nothing to rebuild, the padding
behind every row and the gaps between the stripes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc
from reedsolomon16_amd import _capi
from rows_list_util import (FILL, PATTERN_OF, PLACE, SIZES, case, first_difference, oracle_rows, pair_tables,
                            rows_list_plan, stripe, views)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (16, 2100, 100) is n = 4096: beyond the direct tier's gate, every stripe on its own
GEOMS = [(8, 10, 4), (8, 100, 28), (8, 128, 128), (16, 2, 1), (16, 3, 7), (16, 37, 9), (16, 128, 32), (16, 300, 300),
         (16, 2100, 100)]
# (knob, value) on top of the defaults, or "none": required = NULL
CONFIGS = [("rows_direct", -1), ("rows_direct", 0), ("rows_direct", 1), ("unit_width", 0), ("unit_width", 1),
           ("rows_list", 0), "none"]


def NS():
    """The C-ABI handle of torch's current stream: the calls stay ordered with torch's own work."""
    return rs.codec._stream_handle(None)


def check(buf, want, where, total, what):
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        raise AssertionError("%s: %s" % (what, first_difference(got, want, where, total)))


def test_layout():
    """The list has the shape the other tests are meant to cover."""
    pr, rq = pair_tables(8, 10, 4)
    where, before, want = case(8, 10, 4, pr, rq)
    offs = [w[0] for w in where]
    assert offs != sorted(offs)
    assert {w[1] - w[2] for w in where} >= {0, 64} and any(w[1] == 2 * w[2] for w in where)
    spans = sorted((off, off + 13 * st + S) for off, st, S in where)
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))  # disjoint, with gaps
    assert spans[0][0] > 0 and spans[-1][1] < before.size
    # the expectation itself: a stripe with nothing missing, and a missing row nobody asked for, stay as they were
    z0 = PATTERN_OF.index(0)
    off, st, S = where[z0]
    assert np.array_equal(before[off: off + 13 * st + S], want[off: off + 13 * st + S])
    z3 = PATTERN_OF.index(3)
    off, st, S = where[z3]
    unwanted = np.flatnonzero(~pr[3] & ~rq[3])
    assert unwanted.size and all((want[off + i * st: off + i * st + S] == FILL).all() for i in unwanted)
    assert not np.array_equal(before, want)


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: c if isinstance(c, str) else "%s%+d" % c)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "gf%d-%d+%d" % g)
def test_list_matches_oracle(geom, config, paths):
    bits, k, p = geom
    pr, rq = pair_tables(bits, k, p)
    if config == "none":
        rq = None
    else:
        paths(*config)
    where, before, want = case(bits, k, p, pr, rq)
    c = rs.ReedSolomon(k, p, bits)
    buf = torch.from_numpy(np.array(before)).to(DEV)
    c.reconstruct_rows_dev_list(views(buf, where, k + p), pr, rq, PATTERN_OF)
    torch.cuda.synchronize()
    check(buf, want, where, k + p, "gf%d %d+%d %s" % (bits, k, p, config))
    c.close()


SOME = [(8, 10, 4), (8, 100, 28), (16, 37, 9), (16, 128, 32), (16, 300, 300), (16, 2100, 100)]


@pytest.mark.parametrize("geom", SOME, ids=lambda g: "gf%d-%d+%d" % g)
def test_each_stripe_equals_the_batch_call_alone(geom):
    """Stripe by stripe what rs_reconstruct_rows_dev_batch writes for that
    stripe alone (nstripes = 1, its base, stride, size and pair) on a twin buffer."""
    bits, k, p = geom
    total = k + p
    pr, rq = pair_tables(bits, k, p)
    where, before, _ = case(bits, k, p, pr, rq)
    buf = torch.from_numpy(np.array(before)).to(DEV)
    twin = buf.clone()
    c = rs.ReedSolomon(k, p, bits)
    c.reconstruct_rows_dev_list(views(buf, where, total), pr, rq, PATTERN_OF)
    c2 = rs.ReedSolomon(k, p, bits)
    for z, (off, st, S) in enumerate(where):
        q = PATTERN_OF[z]
        alone = torch.as_strided(twin, (1, total, S), (total * st, st, 1), off)
        c2.reconstruct_rows_dev_batch(alone, pr[q], rq[q])
    torch.cuda.synchronize()
    assert torch.equal(buf, twin)
    c.close()
    c2.close()


@pytest.mark.parametrize("knob", [-1, 0, 1])
@pytest.mark.parametrize("geom", [(8, 10, 4), (16, 37, 9), (16, 128, 32), (16, 300, 300)], ids=lambda g: "gf%d-%d+%d" % g)
def test_an_inconsistent_stripe_follows_the_oracle(paths, geom, knob):
    """Stripe 3 (pair P4, 2112 bytes) has one of its present rows tampered, so
    its rows are no codeword: its wanted rows are what the oracle's Reconstruct
    makes of the tampered rows, each differs from the clean case, and the
    neighbours are unaffected."""
    bits, k, p = geom
    paths("rows_direct", knob)
    pr, rq = pair_tables(bits, k, p)
    assert PATTERN_OF[3] == 4
    rows = np.flatnonzero(pr[4])
    bad = int(rows[np.random.default_rng(bits + k + p).integers(0, rows.size)])
    where, before, want = case(bits, k, p, pr, rq, tamper={3: bad})
    clean = oracle_rows(bits, k, p, SIZES[3], 3, pr[4])
    dirty = oracle_rows(bits, k, p, SIZES[3], 3, pr[4], bad)
    wanted = np.flatnonzero(~pr[4] & rq[4])
    assert wanted.size and all(not np.array_equal(clean[i], dirty[i]) for i in wanted)
    c = rs.ReedSolomon(k, p, bits)
    buf = torch.from_numpy(np.array(before)).to(DEV)
    c.reconstruct_rows_dev_list(views(buf, where, k + p), pr, rq, PATTERN_OF)
    torch.cuda.synchronize()
    check(buf, want, where, k + p, "tampered, rows_direct=%d" % knob)
    c.close()


def erase(total, rows):
    pr = np.ones(total, bool)
    pr[list(rows)] = False
    return pr


def test_mixed_row_counts_in_one_call(paths):
    """40+40 under rows_direct = 1: t = 1, 2, 3, 5, 8 and 11 wanted rows, each
    stripe of another size, in one call: five launches of the list kernel for
    t <= 8 and t = 11 as 6 + 5, its stripe in two lists."""
    bits, k, p = 16, 40, 40
    total = k + p
    ts = [1, 2, 3, 5, 8, 11]
    sizes = [4160, 64, 8256, 192, 2112, 4096]
    rng = np.random.default_rng(4040)
    pr = np.stack([erase(total, rng.choice(total, t, replace=False)) for t in ts])
    rq = np.ones_like(pr)
    paths("rows_direct", 1)
    where, before, want = case(bits, k, p, pr, rq, pattern_of=list(range(6)), sizes=sizes, place=[3, 5, 0, 2, 4, 1],
                               tag="mixed")
    c = rs.ReedSolomon(k, p, bits)
    buf = torch.from_numpy(np.array(before)).to(DEV)
    c.reconstruct_rows_dev_list(views(buf, where, total), pr, rq, list(range(6)))
    torch.cuda.synchronize()
    check(buf, want, where, total, "40+40 mixed t")
    c.close()


def test_direct_and_other_stripes_in_one_call():
    """128+32, automatic: t = 1 stripes go through the list kernel, a stripe of
    32 erasures that wants all of them goes on its own, between them."""
    bits, k, p = 16, 128, 32
    total = k + p
    rng = np.random.default_rng(12832)
    pr = np.stack([erase(total, [5]), erase(total, rng.choice(total, 32, replace=False)), erase(total, [total - 1])])
    pattern_of = [0, 2, 1, 0, 2]
    sizes = [192, 4160, 1088, 8256, 64]
    where, before, want = case(bits, k, p, pr, None, pattern_of=pattern_of, sizes=sizes, place=[4, 2, 0, 3, 1], tag="c4mix")
    c = rs.ReedSolomon(k, p, bits)
    buf = torch.from_numpy(np.array(before)).to(DEV)
    c.reconstruct_rows_dev_list(views(buf, where, total), pr, None, pattern_of)
    torch.cuda.synchronize()
    check(buf, want, where, total, "128+32 mixed tiers")
    c.close()


def test_a_list_across_the_ring_slot_cut():
    """The library's entry limit plus 3000 stripes of 2+1 x 64 bytes, one
    8256-byte stripe in the middle, three one-erasure pairs in rotation.  Every
    small stripe holds the same bytes, so the expected image is a tile."""
    bits, k, p, S, BIG = 16, 2, 1, 64, 8256
    code, limit, _, _ = rows_list_plan(bits, -1, [64], [1])
    assert code == 0
    n = (limit + 3000) // 6 * 6  # two halves, each a whole number of rotations
    half, small = n // 2, (k + p) * S
    pr = ~np.eye(3, dtype=bool)  # pair q: row q is missing
    full_s, full_b = stripe(bits, k, p, S, 0), stripe(bits, k, p, BIG, 0)
    for q in range(3):  # the oracle rebuilds what was there
        assert np.array_equal(oracle_rows(bits, k, p, S, 0, pr[q])[q], full_s[q])
    assert np.array_equal(oracle_rows(bits, k, p, BIG, 0, pr[half % 3])[half % 3], full_b[half % 3])
    three = np.stack([full_s] * 3)
    holes = three.copy()
    for q in range(3):
        holes[q, q] = FILL
    big_holes = np.array(full_b)
    big_holes[half % 3] = FILL

    def image(t, b):
        return np.concatenate([np.tile(t, (half // 3, 1, 1)).ravel(), b.ravel(), np.tile(t, (half // 3, 1, 1)).ravel(),
                               np.full(256, FILL, np.uint8)])

    assert half % 3 == 0
    buf = torch.from_numpy(image(holes, big_holes)).to(DEV)
    want = torch.from_numpy(image(three, full_b)).to(DEV)
    base = buf.data_ptr()
    rec = np.zeros(n + 1, dtype=[("base", "<u8"), ("stride", "<u8"), ("size", "<u8")])
    z = np.arange(n + 1, dtype=np.uint64)
    rec["base"] = base + np.where(z <= half, z * small, (z - 1) * small + (k + p) * BIG)
    rec["stride"], rec["size"] = S, S
    rec["stride"][half], rec["size"][half] = BIG, BIG
    arr = (_capi.Stripe * (n + 1)).from_buffer(rec)
    # the second half's rotation starts again at pair 0, as its tile does
    of = np.where(z <= half, z % 3, (z - 1) % 3).astype(np.uint32)
    assert of[half] == half % 3
    table = np.ascontiguousarray(pr.astype(np.uint8))
    c = rs.ReedSolomon(k, p, bits)
    assert n + 1 > limit
    assert c._L.rs_reconstruct_rows_dev_list(c._h, arr, n + 1, table.ctypes.data_as(C.POINTER(C.c_uint8)), None, 3,
                                             of.ctypes.data_as(C.POINTER(C.c_uint32)), NS()) == 0
    assert torch.equal(buf, want)
    c.close()


def test_two_calls_with_different_tables_back_to_back():
    """Two calls with different tables on a side stream with no host wait
    between, then one check of both: the first call's set must outlive its
    launches."""
    bits, k, p = 16, 37, 9
    total = k + p
    pr, rq = pair_tables(bits, k, p)
    where, before, want = case(bits, k, p, pr, rq)
    pr2 = pr.copy()
    pr2[1] = erase(total, [3, 40])
    pr2[4] = erase(total, [0, 1, 2, 44])
    where2, before2, want2 = case(bits, k, p, pr2, None, tag="second")
    c = rs.ReedSolomon(k, p, bits)
    buf = torch.from_numpy(np.array(before)).to(DEV)
    buf2 = torch.from_numpy(np.array(before2)).to(DEV)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c.reconstruct_rows_dev_list(views(buf, where, total), pr, rq, PATTERN_OF, stream=st)
        c.reconstruct_rows_dev_list(views(buf2, where2, total), pr2, None, PATTERN_OF, stream=st)
    st.synchronize()
    check(buf, want, where, total, "first call")
    check(buf2, want2, where2, total, "second call")
    c.close()


@pytest.mark.parametrize("null_stream", [False, True], ids=["side-stream", "null-stream"])
@pytest.mark.parametrize("geom", [(8, 10, 4), (16, 128, 32)], ids=lambda g: "gf%d-%d+%d" % g)
def test_stream_order(geom, null_stream):
    """The call is ordered on its stream: the rows it reads are made by the
    kernel before it and its rows are read by the kernel after it, with no
    host wait between."""
    bits, k, p = geom
    pr, rq = pair_tables(bits, k, p)
    where, before, want = case(bits, k, p, pr, rq)
    c = rs.ReedSolomon(k, p, bits)
    masked = torch.from_numpy(before ^ 0x5A).to(DEV)
    buf = torch.empty_like(masked)
    stripes = views(buf, where, k + p)
    torch.cuda.synchronize()
    st = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    if null_stream:
        assert rs.codec._stream_handle(st) == rs.codec.RS_NULL_STREAM
    with torch.cuda.stream(st):
        torch.bitwise_xor(masked, 0x5A, out=buf)
        c.reconstruct_rows_dev_list(stripes, pr, rq, PATTERN_OF, stream=st)
        got = buf.clone()
    st.synchronize()
    check(got, want, where, k + p, "stream order")
    c.close()


def test_rows_more_than_4_gib_apart():
    """2+1, 4160 bytes, row stride 2.25 GiB: the rows of a stripe lie at 0,
    2.25 and 4.5 GiB of an unfilled buffer.  One stripe rebuilds its row at
    4.5 GiB, a second stripe in the same call rebuilds its row 0 from its far
    rows.  Only the rows are written and read."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip("needs 6 GiB of free device memory, %.1f GiB are free" % (free / 2**30))
    bits, k, p, S = 16, 2, 1, 4160
    stride = 9 << 28  # 2.25 GiB
    second = 8192     # the second stripe's rows lie this far behind the first's
    buf = torch.empty(2 * stride + second + S, dtype=torch.uint8, device=DEV)
    a, b = stripe(bits, k, p, S, 0), stripe(bits, k, p, S, 1)
    pr = np.stack([erase(3, [2]), erase(3, [0])])
    assert np.array_equal(oracle_rows(bits, k, p, S, 0, pr[0])[2], a[2])
    assert np.array_equal(oracle_rows(bits, k, p, S, 1, pr[1])[0], b[0])
    va = torch.as_strided(buf, (3, S), (stride, 1), 0)
    vb = torch.as_strided(buf, (3, S), (stride, 1), second)
    ha, hb = np.array(a), np.array(b)
    ha[2], hb[0] = FILL, FILL
    va.copy_(torch.from_numpy(ha))
    vb.copy_(torch.from_numpy(hb))
    c = rs.ReedSolomon(k, p, bits)
    c.reconstruct_rows_dev_list([va, vb], pr, None, [0, 1])
    torch.cuda.synchronize()
    assert np.array_equal(va.cpu().numpy(), a)
    assert np.array_equal(vb.cpu().numpy(), b)
    c.close()
    del va, vb, buf
    torch.cuda.empty_cache()
