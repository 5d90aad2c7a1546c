"""CPU tests of rs_update_dev_batch_list's host side: its error rules, which are
all decided before any device call (on codecs that never touch a device, with
fake device pointers), the launch plan the call would make
(rs_debug_update_list_plan) and the Python mirror's type checks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from reedsolomon16_amd import _capi

FAKE = 0x10000  # a non-NULL "device pointer": every call below must fail before it is used
INV, NO_DATA, BAD_SIZE, PANIC = 53, 4, 6, 50
K, P, S = 4, 2, 128


@pytest.fixture(scope="module")
def codecs():
    one = rs.New16(K, P)
    multi = rs.New16(K, P, devices=[0, 0])
    yield one, multi
    one.close()
    multi.close()


def call(c, base=FAKE, rs_=S, ss=(K + P) * S, ns=3, stripes=(0, 2, 2), idx=(1, 0, 3), nrows=None, new=FAKE * 2, nrs=S,
         size=S):
    L = _capi.lib()
    zarr = (C.c_uint32 * max(len(stripes), 1))(*stripes) if stripes is not None else None
    iarr = (C.c_int * max(len(idx), 1))(*idx) if idx is not None else None
    n = (len(idx) if idx is not None else 1) if nrows is None else nrows
    return L.rs_update_dev_batch_list(c, base, rs_, ss, ns, zarr, iarr, n, new, nrs, size, None)


def check_rules(h):
    """The error table of the header, in its order; each case breaks one rule."""
    # 1. NULL arguments
    assert call(None) == INV
    assert call(h, base=None) == INV
    assert call(h, stripes=None) == INV
    assert call(h, idx=None) == INV
    assert call(h, new=None) == INV
    # 2. counts beyond INT32_MAX (decided before the arrays are read)
    assert call(h, ns=2**31) == INV
    assert call(h, nrows=2**31) == INV
    # 4. the list itself
    assert call(h, stripes=(0, 3, 2)) == INV      # stripe_of[e] >= nstripes
    assert call(h, idx=(1, K, 3)) == INV          # idx_of[e] outside [0, k)
    assert call(h, idx=(1, -1, 3)) == INV
    assert call(h, stripes=(0, 2, 2), idx=(1, 3, 3)) == INV    # the same (stripe, index) pair twice
    assert call(h, stripes=(2, 0, 2), idx=(3, 1, 3)) == INV    # ... not adjacent in the list
    assert call(h, ns=0) == INV                   # no stripe can be named
    # 5., 6. the shard size
    assert call(h, size=0) == NO_DATA
    assert call(h, size=100) == BAD_SIZE
    # 7. strides
    assert call(h, rs_=S - 64) == INV
    assert call(h, nrs=S - 64) == INV
    assert call(h, ss=(K + P) * S - 64) == INV
    # ... and their order: the list is checked before the size, the size before the strides
    assert call(h, idx=(1, K, 3), size=0) == INV
    assert call(h, size=0, rs_=0) == NO_DATA
    assert call(h, size=100, rs_=64) == BAD_SIZE


def test_error_table_in_order(codecs):
    one, _ = codecs
    check_rules(one._h)
    # one stripe needs no stripe stride
    assert call(one._h, ns=1, stripes=(), idx=(), ss=0) == 0
    assert call(one._h, ns=1, stripes=(), idx=(), ss=0, size=0) == NO_DATA


def test_multi_device_codec_is_refused(codecs):
    _, multi = codecs
    h = multi._h
    # 1. and 2. come first, as on a single-device codec
    assert call(None) == INV
    assert call(h, base=None) == INV
    assert call(h, ns=2**31) == INV
    # 3. a well-formed call, and every later rule, is refused as a multi-device call
    assert call(h) == INV
    assert call(h, size=0) == INV
    assert call(h, size=100) == INV
    assert call(h, stripes=(), idx=()) == INV


def test_empty_list_is_ok_and_launches_nothing(codecs):
    one, _ = codecs
    # fake pointers: a device call would fault; RS_NULL_STREAM and the codec's stream alike
    assert call(one._h, stripes=(), idx=()) == 0
    L = _capi.lib()
    z, i = (C.c_uint32 * 1)(), (C.c_int * 1)()
    assert L.rs_update_dev_batch_list(one._h, FAKE, S, (K + P) * S, 3, z, i, 0, FAKE * 2, S, S,
                                      C.c_void_p(rs.codec.RS_NULL_STREAM)) == 0
    # the checks still come first
    assert call(one._h, stripes=(), idx=(), size=0) == NO_DATA
    assert call(one._h, stripes=(), idx=(), size=100) == BAD_SIZE
    assert call(one._h, stripes=(), idx=(), rs_=64) == INV


def test_panic_geometry_is_refused_before_any_device_call():
    """GF(2^8) 250+6: the reference's encode panics, so there is no generator to update with."""
    c = rs.New8(250, 6)
    L = _capi.lib()
    z, i = (C.c_uint32 * 2)(0, 1), (C.c_int * 2)(3, 249)
    assert L.rs_update_dev_batch_list(c._h, FAKE, 64, 256 * 64, 2, z, i, 2, FAKE * 2, 64, 64, None) == PANIC
    assert L.rs_update_dev_batch_list(c._h, FAKE, 64, 256 * 64, 2, z, i, 0, FAKE * 2, 64, 64, None) == PANIC
    i[1] = 250
    assert L.rs_update_dev_batch_list(c._h, FAKE, 64, 256 * 64, 2, z, i, 2, FAKE * 2, 64, 64, None) == INV
    c.close()


# ---------------------------------------------------------------- the launch plan
def plan(k, nstripes, stripes, idx):
    L = _capi.lib()
    n = len(idx)
    zarr = np.zeros(max(n, 1), np.uint32)
    iarr = np.zeros(max(n, 1), np.int32)
    zarr[:n] = stripes
    iarr[:n] = idx
    nl = C.c_int(-1)
    launches = np.full(3 * max(n, 1), -1, np.int32)
    zs = np.zeros(max(n, 1), np.uint32)
    es = np.zeros(max(n, 1), np.uint32)
    e = L.rs_debug_update_list_plan(k, nstripes, zarr.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    iarr.ctypes.data_as(C.POINTER(C.c_int)), n, C.byref(nl), launches.ctypes.data,
                                    zs.ctypes.data, es.ctypes.data)
    if e:
        return e
    out, g0, e0 = [], 0, 0
    for l in range(nl.value):
        nt, rnd, ng = (int(v) for v in launches[3 * l:3 * l + 3])
        out.append({"nt": nt, "round": rnd, "stripes": [int(z) for z in zs[g0:g0 + ng]],
                    "groups": [[int(x) for x in es[e0 + g * nt:e0 + (g + 1) * nt]] for g in range(ng)]})
        g0 += ng
        e0 += ng * nt
    assert e0 == n
    return out


def split(t):
    """update_f's rule: ceil(t / 8) groups of near-equal size."""
    ng = -(-t // 8)
    return [t // ng + (1 if g < t % ng else 0) for g in range(ng)]


COUNTS = [0, 1, 1, 3, 9, 16, 17, 0]


def shuffled_list(k, counts, seed):
    rng = np.random.default_rng(seed)
    ent = [(z, int(j)) for z, t in enumerate(counts) for j in rng.choice(k, t, replace=False)]
    order = rng.permutation(len(ent))
    return [ent[i][0] for i in order], [ent[i][1] for i in order]


def test_split_rule():
    assert split(9) == [5, 4] and split(16) == [8, 8] and split(17) == [6, 6, 5] and split(8) == [8] and split(1) == [1]


def test_plan_of_the_eight_stripe_list():
    k = 128
    stripes, idx = shuffled_list(k, COUNTS, 7)
    # shuffled: the entries of stripe 5 are neither adjacent nor sorted
    at5 = [e for e, z in enumerate(stripes) if z == 5]
    assert at5 != list(range(at5[0], at5[0] + 16))
    launches = plan(k, len(COUNTS), stripes, idx)
    assert not isinstance(launches, int)

    # no launch names a stripe twice
    for l in launches:
        assert len(set(l["stripes"])) == len(l["stripes"]), l
        assert 1 <= l["nt"] <= 8 and len(l["groups"]) == len(l["stripes"]) >= 1
    # every entry appears in exactly one group, and in a group of its own stripe
    seen = np.zeros(len(idx), int)
    for l in launches:
        for z, g in zip(l["stripes"], l["groups"]):
            for e in g:
                seen[e] += 1
                assert stripes[e] == z
    assert (seen == 1).all()
    # the groups of a stripe have the rule's sizes, in rounds 0, 1, 2, ...
    for z, t in enumerate(COUNTS):
        mine = [(l["round"], l["nt"]) for l in launches for zz in l["stripes"] if zz == z]
        assert sorted(nt for _, nt in mine) == sorted(split(t)), (z, mine)
        assert sorted(r for r, _ in mine) == list(range(len(split(t)))), (z, mine)
    sizes = {z: sorted(l["nt"] for l in launches if z in l["stripes"]) for z in range(8)}
    assert sizes[4] == [4, 5] and sizes[5] == [8, 8] and sizes[6] == [5, 6, 6] and sizes[0] == [] and sizes[7] == []
    # 16 rows: two groups of 8, in two different launches and rounds
    l5 = [n for n, l in enumerate(launches) if 5 in l["stripes"]]
    assert len(l5) == 2 and launches[l5[0]]["round"] != launches[l5[1]]["round"]
    # launches of one stripe are ordered on the stream: the list is in stream
    # order, rounds never go back, and a stripe's launches have rising rounds
    rounds = [l["round"] for l in launches]
    assert rounds == sorted(rounds)
    for z in range(8):
        mine = [l["round"] for l in launches if z in l["stripes"]]
        assert mine == sorted(set(mine))
    # the number of launches, from the rule: one per (round, group size) that occurs
    want = {(g, nt) for t in COUNTS for g, nt in enumerate(split(t))}
    assert len(launches) == len(want)
    assert {(l["round"], l["nt"]) for l in launches} == want
    # stripes 1 and 2 (one row each) share the nt = 1 launch of round 0
    one = [l for l in launches if l["nt"] == 1]
    assert len(one) == 1 and sorted(one[0]["stripes"]) == [1, 2]


def test_plan_checks_the_list():
    assert plan(4, 3, [0, 3], [1, 1]) == INV
    assert plan(4, 3, [0, 2], [1, 4]) == INV
    assert plan(4, 3, [0, 2], [1, -1]) == INV
    assert plan(4, 3, [2, 0, 2], [1, 1, 1]) == INV
    assert plan(0, 3, [0], [0]) == INV
    assert plan(4, 3, [], []) == []
    assert plan(4, 3, [2, 0, 2], [1, 1, 0]) == [
        {"nt": 1, "round": 0, "stripes": [0], "groups": [[1]]},
        {"nt": 2, "round": 0, "stripes": [2], "groups": [[2, 0]]},  # ascending data index
    ]
    L = _capi.lib()
    assert L.rs_debug_update_list_plan(4, 3, None, None, 0, None, None, None, None) == INV


# ---------------------------------------------------------------- the Python mirror
def test_python_mirror_type_errors(codecs):
    one, _ = codecs
    assert callable(rs.ReedSolomon.update_dev_batch_list)
    assert "rs_update_dev_batch_list" in _capi.header_functions()
    assert "rs_debug_update_list_plan" in _capi.header_functions()
    slab = torch.zeros((3, K + P, S), dtype=torch.uint8)
    new = torch.zeros((2, S), dtype=torch.uint8)
    with pytest.raises(TypeError):
        one.update_dev_batch_list(slab, [0, 1], [1, 2], new)  # not on a device
    with pytest.raises(TypeError):
        one.update_dev_batch_list(slab[0], [0, 1], [1, 2], new)  # not a slab
    with pytest.raises(TypeError):
        one.update_dev_batch_list(torch.zeros((3, K + P + 1, S), dtype=torch.uint8), [0, 1], [1, 2], new)
    with pytest.raises(TypeError):
        one.update_dev_batch_list(slab, [0, 1], [1], new)  # lists of different lengths
