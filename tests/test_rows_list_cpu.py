"""CPU tests of rs_reconstruct_rows_dev_list's host side: the error rules and
their order, all decided before any device call (on codecs that never touch a
device, with fake device pointers, so every call below must fail or launch
nothing), and the launch plan of its list kernel (rs_debug_rows_list_plan):
the ranges, one launch per wanted-row count, the unit width, the prefixes, the
ring-slot cut at the library's own limit and the 2^31 workgroup cut.
"""
import ctypes as C

import numpy as np
import pytest

import reedsolomon16_amd as rs
from reedsolomon16_amd import _capi
from rows_list_util import rows_list_plan

FAKE = 0x10000  # a non-NULL "device pointer": never dereferenced here
INV, TOO_FEW, NO_DATA, BAD_SIZE, PANIC = 53, 3, 4, 6, 50
K, P = 4, 2
TOTAL = K + P
GOOD = (FAKE, 128, 128)

ALL = [1] * TOTAL
ONE_GONE = [0] + [1] * (TOTAL - 1)
NONE_PRESENT = [0] * TOTAL                 # rule 2
THREE_PRESENT = [1, 1, 1, 0, 0, 0]         # rule 3: fewer than k = 4

NULL_BASE = (None, 128, 128)               # 1
NO_BYTES = (FAKE, 128, 0)                  # 2
ODD = (FAKE, 128, 100)                     # 4
SHORT_STRIDE = (FAKE, 64, 128)             # 5


def call(h, stripes, table, pattern_of=None, required=None, n=None, npat=None, null=()):
    L = _capi.lib()
    arr = (_capi.Stripe * max(len(stripes), 1))()
    for i, (b, st, S) in enumerate(stripes):
        arr[i] = _capi.Stripe(b, st, S)
    tb = np.ascontiguousarray(np.array(table, np.uint8))
    rq = None if required is None else np.ascontiguousarray(np.array(required, np.uint8))
    of = np.array(list(pattern_of if pattern_of is not None else [0] * len(stripes)) + [0], np.uint32)
    return L.rs_reconstruct_rows_dev_list(
        h, None if "stripes" in null else arr, len(stripes) if n is None else n,
        None if "present" in null else tb.ctypes.data_as(C.POINTER(C.c_uint8)),
        None if rq is None else rq.ctypes.data_as(C.POINTER(C.c_uint8)), tb.shape[0] if npat is None else npat,
        None if "pattern_of" in null else of.ctypes.data_as(C.POINTER(C.c_uint32)), None)


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(K, P)
    multi = rs.New16(K, P, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def test_each_rule(codecs):
    h = codecs[0]._h
    assert call(None, [GOOD], [ONE_GONE]) == INV
    for what in ("stripes", "present", "pattern_of"):
        assert call(h, [GOOD], [ONE_GONE], null=(what,)) == INV
        assert call(h, [], [ONE_GONE], null=(what,)) == INV  # ... with nothing to do as well
    assert call(h, [GOOD], [ONE_GONE], n=2**31) == INV       # decided before the list is read
    assert call(h, [GOOD], [ONE_GONE], npat=0) == INV
    assert call(h, [GOOD], [ONE_GONE], npat=65537) == INV
    assert call(h, [GOOD, GOOD], [ONE_GONE, ALL], pattern_of=[1, 2]) == INV
    assert call(h, [GOOD, NULL_BASE], [ONE_GONE]) == INV
    assert call(h, [GOOD, NO_BYTES], [ONE_GONE]) == NO_DATA
    assert call(h, [GOOD], [ONE_GONE, NONE_PRESENT]) == NO_DATA
    assert call(h, [GOOD], [ONE_GONE, THREE_PRESENT]) == TOO_FEW   # a row no stripe names
    assert call(h, [GOOD, ODD], [ONE_GONE]) == BAD_SIZE
    assert call(h, [SHORT_STRIDE, GOOD], [ONE_GONE]) == INV
    assert call(h, [GOOD, (FAKE, 1 << 43, 1 << 42)], [ONE_GONE]) == INV  # no grid covers 2^42 bytes


def test_rule_order(codecs):
    """Each rule runs over the whole list and the whole table before the
    next: an earlier rule broken late wins over a later rule broken early."""
    h = codecs[0]._h
    assert call(h, [(None, 128, 0)], [ONE_GONE]) == INV                         # 1 before 2, in one stripe
    assert call(h, [NO_BYTES, NULL_BASE], [ONE_GONE]) == INV                    # 1 before 2
    assert call(h, [NO_BYTES, GOOD], [NONE_PRESENT], pattern_of=[0, 1]) == INV  # 1 before 2 (table)
    assert call(h, [GOOD, NO_BYTES], [THREE_PRESENT]) == NO_DATA                # 2 before 3
    assert call(h, [GOOD], [THREE_PRESENT, ALL, NONE_PRESENT]) == NO_DATA       # 2 over the whole table before 3
    assert call(h, [ODD], [ALL, THREE_PRESENT]) == TOO_FEW                      # 3 before 4, by an unnamed row
    assert call(h, [ODD, NO_BYTES], [ALL]) == NO_DATA                           # 2 before 4
    assert call(h, [SHORT_STRIDE, ODD], [ALL]) == BAD_SIZE                      # 4 before 5
    assert call(h, [(FAKE, 64, 100)], [ALL]) == BAD_SIZE                        # ... in one stripe
    assert call(h, [SHORT_STRIDE], [ALL, THREE_PRESENT]) == TOO_FEW             # 3 before 5
    # the errors do not depend on whether anything is to be rebuilt
    assert call(h, [ODD], [ALL]) == BAD_SIZE
    assert call(h, [SHORT_STRIDE], [ALL]) == INV
    # 6 comes last
    panics = rs.New8(250, 6)  # 8 + 250 > 256: the reference's reconstruct panics
    try:
        hp, full = panics._h, [[1] * 256]
        assert call(hp, [GOOD], full) == PANIC
        assert call(hp, [], full) == PANIC                   # the geometry is refused even with nothing to do
        assert call(hp, [GOOD, SHORT_STRIDE], full) == INV   # 5 before 6
        assert call(hp, [GOOD, ODD], full) == BAD_SIZE
        assert call(hp, [GOOD], [[1] * 249 + [0] * 7]) == TOO_FEW
        assert call(hp, [GOOD, NO_BYTES], full) == NO_DATA
        assert call(hp, [NULL_BASE], full) == INV
    finally:
        panics.close()


def test_multi_device_codec_is_refused(codecs):
    h = codecs[1]._h
    assert call(h, [GOOD], [ONE_GONE]) == INV
    assert call(h, [], [ONE_GONE]) == INV
    assert call(h, [NO_BYTES], [ONE_GONE]) == INV   # rule 1 comes first
    assert call(h, [GOOD], [THREE_PRESENT]) == INV
    assert call(h, [ODD], [ALL]) == INV


def test_nothing_to_do(codecs):
    """No stripes, and a list in which nothing is missing or nothing missing is
    required: RS_OK, and nothing launched -- the codec has no device half and
    the pointers are fake, so a launch could not have ended well."""
    c = codecs[0]
    h = c._h
    assert call(h, [], [ONE_GONE]) == 0
    assert call(h, [NO_BYTES], [ONE_GONE], n=0) == 0  # nothing is read
    assert call(h, [GOOD, (FAKE, 4160, 4160)], [ALL, ONE_GONE], pattern_of=[0, 0]) == 0
    nothing_required = [[0] * TOTAL, [0] * TOTAL]
    assert call(h, [GOOD, GOOD], [ALL, ONE_GONE], pattern_of=[0, 1], required=nothing_required) == 0
    present_required = [ALL, ONE_GONE]  # required flags on present rows only
    assert call(h, [GOOD, GOOD], [ALL, ONE_GONE], pattern_of=[0, 1], required=present_required) == 0
    assert c.reconstruct_rows_dev_list([], [ONE_GONE], None, [], stream=0) is None


# ---------------------------------------------------------------- the plan

WIDE = {8: 4096, 16: 8192}
RAGGED = [64, 192, 2048, 2112, 4096, 4160, 8192, 8256, 64, 64 * 700, 128]
RAGGED_T = [1, 3, 1, 8, 3, 1, 1, 3, 8, 1, 2]


def check_plan(bits, unit_width, sizes, wanted, launches, pres):
    """What every plan must satisfy; returns the launches by range."""
    ranges, at = {}, 0
    for l, pre in zip(launches, pres):
        e0, e1, t, n, wgb, nwg, o_ent, o_pre, nbytes = (int(x) for x in l)
        ranges.setdefault((e0, e1), []).append(l)
        idx = [i for i in range(e0, e1) if wanted[i] == t]
        assert n == len(idx) and n > 0
        assert wgb in (WIDE[bits], WIDE[bits] // 2)
        if unit_width >= 0:
            assert wgb == WIDE[bits] >> unit_width
        wgs = [-(-sizes[i] // wgb) for i in idx]
        assert pre[0] == 0 and pre[-1] == nwg == sum(wgs) and nwg < 2**31
        assert (np.diff(pre) == wgs).all() and (np.diff(pre) > 0).all()  # strictly ascending
        if unit_width < 0:
            wide = sum(-(-sizes[i] // WIDE[bits]) for i in idx)
            assert (wgb == WIDE[bits] // 2) == (wide < 1024)
        assert o_ent % 256 == 0 and o_pre % 256 == 0 and o_ent + 32 * n <= o_pre and o_pre + 4 * (n + 1) <= nbytes
    keys = sorted(ranges)
    for (e0, e1) in keys:  # the ranges tile the entries in order; a range has one launch per count that occurs
        assert e0 == at and e1 > e0
        at = e1
        ts = [int(l[2]) for l in ranges[(e0, e1)]]
        assert ts == sorted(set(wanted[e0:e1]))
        spans = sorted((int(l[6]), int(l[7]) + 4 * (int(l[3]) + 1)) for l in ranges[(e0, e1)])
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))  # the launches' arrays do not overlap in the slot
    assert at == len(sizes)
    return [ranges[k] for k in keys]


@pytest.mark.parametrize("unit_width", [-1, 0, 1])
@pytest.mark.parametrize("bits", [8, 16])
def test_plan_of_a_ragged_list(bits, unit_width):
    code, limit, launches, pres = rows_list_plan(bits, unit_width, RAGGED, RAGGED_T)
    assert code == 0 and limit > 100_000
    by_range = check_plan(bits, unit_width, RAGGED, RAGGED_T, launches, pres)
    assert len(by_range) == 1 and [int(l[2]) for l in by_range[0]] == [1, 2, 3, 8]
    # few workgroups: the automatic width is the narrow one
    if unit_width < 0:
        assert all(int(l[4]) == WIDE[bits] // 2 for l in launches)
    # a small entry limit cuts the same list into ranges of that many entries
    code, _, launches, pres = rows_list_plan(bits, unit_width, RAGGED, RAGGED_T, max_entries=4)
    assert code == 0
    by_range = check_plan(bits, unit_width, RAGGED, RAGGED_T, launches, pres)
    assert [(int(r[0][0]), int(r[0][1])) for r in by_range] == [(0, 4), (4, 8), (8, 11)]


@pytest.mark.parametrize("bits", [8, 16])
def test_automatic_width_on_either_side_of_1024_workgroups(bits):
    """The rule is applied per launch, to the launch's own total."""
    w = WIDE[bits]
    # t = 1: 1023 wide workgroups (narrow); t = 2: 1024 (wide); one list
    sizes = [w * 1000, w * 23, w * 1000, w * 24]
    wanted = [1, 1, 2, 2]
    code, _, launches, pres = rows_list_plan(bits, -1, sizes, wanted)
    assert code == 0
    check_plan(bits, -1, sizes, wanted, launches, pres)
    assert [(int(l[2]), int(l[4]), int(l[5])) for l in launches] == [(1, w // 2, 2046), (2, w, 1024)]
    # a ragged tail counts as a workgroup: 1022 full ones and two tails are 1024
    sizes = [w * 1021 + 64, w + 64]
    code, _, launches, pres = rows_list_plan(bits, -1, sizes, [5, 5])
    assert code == 0 and [(int(l[4]), int(l[5])) for l in launches] == [(w, 1024)]
    sizes = [w * 1021 + 64, w]
    code, _, launches, pres = rows_list_plan(bits, -1, sizes, [5, 5])
    assert code == 0 and [(int(l[4]), int(l[5])) for l in launches] == [(w // 2, 2045)]


def test_slot_cut_at_the_librarys_limit():
    """The library's entry limit fits one ring slot; one entry more starts a second range."""
    code, limit, _, _ = rows_list_plan(16, -1, [64], [1])
    assert code == 0 and 1000 < limit < (4 << 20) // 36
    wanted = [1 + i % 8 for i in range(limit + 1)]
    sizes = [64] * (limit + 1)
    code, _, launches, pres = rows_list_plan(16, -1, sizes[:limit], wanted[:limit])
    assert code == 0
    by_range = check_plan(16, -1, sizes[:limit], wanted[:limit], launches, pres)
    assert len(by_range) == 1 and len(by_range[0]) == 8 and int(launches[0][8]) <= 4 << 20
    code, _, launches, pres = rows_list_plan(16, -1, sizes, wanted)
    assert code == 0
    by_range = check_plan(16, -1, sizes, wanted, launches, pres)
    assert [(int(r[0][0]), int(r[0][1])) for r in by_range] == [(0, limit), (limit, limit + 1)]
    assert len(by_range[1]) == 1 and int(by_range[1][0][2]) == wanted[limit]
    assert max(int(l[8]) for l in launches) <= 4 << 20


def test_workgroup_cut_from_sizes_alone():
    """2^40 bytes a shard are 2^29 narrow GF(2^8) workgroups: three entries of
    one wanted-row count fit a launch of fewer than 2^31, the fourth starts a
    new range.  No memory stands behind these sizes."""
    sizes = [1 << 40] * 10
    wanted = [1, 1, 1, 2, 1, 1, 2, 2, 2, 2]
    code, _, launches, pres = rows_list_plan(8, 1, sizes, wanted)
    assert code == 0
    by_range = check_plan(8, 1, sizes, wanted, launches, pres)
    assert [(int(r[0][0]), int(r[0][1])) for r in by_range] == [(0, 4), (4, 9), (9, 10)]
    assert int(launches[0][5]) == 3 << 29
    # at the wide unit everything fits one range
    code, _, launches, pres = rows_list_plan(8, 0, sizes, wanted)
    assert code == 0 and len(check_plan(8, 0, sizes, wanted, launches, pres)) == 1
    # one entry of 2^31 workgroups or more is refused
    assert rows_list_plan(8, 1, [1 << 42], [1])[0] == INV
    assert rows_list_plan(8, 1, [(1 << 42) - 2048], [1])[0] == 0


def test_plan_arguments():
    assert rows_list_plan(12, -1, [64], [1])[0] == INV
    assert rows_list_plan(8, 2, [64], [1])[0] == INV
    assert rows_list_plan(8, -1, [0], [1])[0] == INV
    assert rows_list_plan(8, -1, [100], [1])[0] == INV
    assert rows_list_plan(8, -1, [64], [0])[0] == INV
    assert rows_list_plan(8, -1, [64], [9])[0] == INV
    code, limit, launches, pres = rows_list_plan(8, -1, [], [])
    assert code == 0 and limit > 0 and len(launches) == 0
