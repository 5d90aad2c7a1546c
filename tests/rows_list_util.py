"""Helpers of the rs_reconstruct_rows_dev_list tests: the six-pair table, the
stripes of a ragged list laid out in one buffer, and the expected image after
a call -- a fresh oracle's Reconstruct per stripe in the wanted rows, every
other byte as it was.  Everything computed here is cached and never written.
"""
import ctypes as C

import numpy as np

from oracle import orc
from reedsolomon16_amd import _capi

FILL = 0xA5
# One unit, a ragged block, and the workgroup span of each of the four unit
# widths (GF(2^8) narrow 2048 / wide 4096, GF(2^16) narrow 4096 / wide 8192)
# with that span plus 64.
SIZES = [64, 192, 2048, 2112, 4096, 4160, 8192, 8256, 64]
PLACE = [4, 0, 7, 2, 8, 5, 1, 6, 3]  # the stripes' order in memory: not the list's
PATTERN_OF = [2, 0, 1, 4, 2, 3, 1, 1, 4]


def row_stride(z, S):
    return (S, S + 64, 2 * S)[z % 3]


def pair_tables(bits, k, p):
    """([6, k+p] present, [6, k+p] required).  P0 nothing missing; P1 one data
    row missing and required (t = 1); P2 min(p, 9) rows missing, data and parity
    mixed where p >= 2, all required; P3 parity rows missing, two of them
    required; P4 = P2's erasures shifted by one index with only its first three
    missing rows required; P5 a copy of P2 that no stripe names.  Required
    flags on present rows are set here and there: they are ignored."""
    rng = np.random.default_rng(bits * 103 + k * 7 + p)
    total = k + p
    pr = np.ones((6, total), bool)
    rq = np.zeros((6, total), bool)
    rq[0] = True
    pr[1, int(rng.integers(0, k))] = False
    rq[1] = True
    n2 = min(p, 9)
    d = int(rng.integers(0, k))
    if n2 >= 2:
        q = k + int(rng.integers(0, p))
        rest = [i for i in range(total) if i not in (d, q)]
        p2 = np.array(sorted([d, q] + rng.choice(rest, n2 - 2, replace=False).tolist()))
    else:
        p2 = np.array([d])
    pr[2, p2] = False
    rq[2] = True
    p3 = k + np.sort(rng.choice(p, min(p, 3), replace=False))
    pr[3, p3] = False
    rq[3, p3[-2:]] = True
    rq[3, 0] = True  # present: ignored
    p4 = np.sort((p2 + 1) % total)
    pr[4, p4] = False
    rq[4, p4[:3]] = True
    rq[4, int(np.flatnonzero(pr[4])[-1])] = True  # present: ignored
    pr[5], rq[5] = pr[2], rq[2]
    assert (pr.sum(axis=1) >= k).all()
    want = ~pr & rq
    assert want[1].sum() == 1 and want[2].sum() == n2 and want[3].sum() == min(p, 2) and want[4].sum() == min(n2, 3)
    return pr, rq


_stripes = {}
_oracle = {}


def stripe(bits, k, p, S, z, tamper=None):
    """Encoded stripe z (k+p rows); tamper: index of a row replaced by other
    bytes, so the rows are no codeword."""
    key = (bits, k, p, S, z, tamper)
    if key not in _stripes:
        rng = np.random.default_rng(bits * 7919 + k * 131 + p * 17 + S + 1000003 * z)
        data = rng.integers(0, 256, (k, S), dtype=np.uint8)
        full = np.concatenate([data, orc.encode(bits, k, p, data)])
        if tamper is not None:
            full[tamper] ^= rng.integers(1, 256, S, dtype=np.uint8)
        full.setflags(write=False)
        _stripes[key] = full
    return _stripes[key]


def oracle_rows(bits, k, p, S, z, present, tamper=None):
    """{index: row} of every missing row as a fresh oracle's Reconstruct rebuilds it."""
    key = (bits, k, p, S, z, tamper, present.tobytes())
    if key not in _oracle:
        full = stripe(bits, k, p, S, z, tamper)
        lst = [np.array(full[i]) if present[i] else None for i in range(k + p)]
        e, out = orc.Oracle(bits, k, p).reconstruct(lst, recover_all=True)
        assert e == 0, e
        _oracle[key] = {i: out[i] for i in range(k + p) if not present[i]}
    return _oracle[key]


def layout(total, sizes, place):
    """Per stripe (offset, row stride, size) with the stripes in `place` order
    in memory and a gap after each, and the buffer length."""
    where, at = [None] * len(sizes), 64
    for z in place:
        S = sizes[z]
        st = row_stride(z, S)
        where[z] = (at, st, S)
        at += (total - 1) * st + S + 64 * (1 + z % 3)
    return where, at + 64


_cases = {}


def case(bits, k, p, pr, rq, pattern_of=PATTERN_OF, sizes=SIZES, place=PLACE, tamper=None, tag=""):
    """(where, before, want): the buffer before the call (the present rows of
    every stripe, FILL everywhere else) and the expected image after it.  rq
    None: every missing row is wanted.  tamper: {stripe: row}.  Cached under
    (geometry, tag, rq is None, tamper): a tag names the tables and the list."""
    key = (bits, k, p, tag, rq is None, tuple(sorted((tamper or {}).items())))
    if key in _cases:
        return _cases[key]
    total = k + p
    where, length = layout(total, sizes, place)
    before = np.full(length, FILL, np.uint8)
    for z, (off, st, S) in enumerate(where):
        full = stripe(bits, k, p, S, z, (tamper or {}).get(z))
        for i in np.flatnonzero(pr[pattern_of[z]]):
            before[off + i * st: off + i * st + S] = full[i]
    want = before.copy()
    for z, (off, st, S) in enumerate(where):
        q = pattern_of[z]
        wanted = ~pr[q] if rq is None else ~pr[q] & rq[q]
        if wanted.any():
            rows = oracle_rows(bits, k, p, S, z, pr[q], (tamper or {}).get(z))
            for i in np.flatnonzero(wanted):
                want[off + i * st: off + i * st + S] = rows[i]
    before.setflags(write=False)
    want.setflags(write=False)
    _cases[key] = (where, before, want)
    return _cases[key]


def views(buf, where, total):
    import torch

    return [torch.as_strided(buf, (total, S), (st, 1), off) for off, st, S in where]


def first_difference(got, want, where, total):
    """Where two images differ, for an assertion message."""
    at = int(np.flatnonzero(got != want)[0])
    for z, (off, st, S) in enumerate(where):
        if off <= at < off + (total - 1) * st + S:
            return "byte %d: stripe %d row %d column %d" % (at, z, (at - off) // st, (at - off) % st)
    return "byte %d: outside every stripe" % at


def rows_list_plan(bits, unit_width, sizes, wanted, max_entries=0):
    """rs_debug_rows_list_plan: (code, entry limit, launches [n, 9], prefixes: one array per launch)."""
    L = _capi.lib()
    n = len(sizes)
    sz = (C.c_size_t * max(n, 1))(*sizes)
    wt = (C.c_int * max(n, 1))(*wanted)
    limit, nl = C.c_size_t(0), C.c_int(-1)
    code = L.rs_debug_rows_list_plan(bits, unit_width, sz, wt, n, max_entries, C.byref(limit), C.byref(nl), None, None)
    if code:
        return code, limit.value, None, None
    launches = np.zeros((max(nl.value, 1), 9), np.uint64)
    pre = np.full(n + nl.value + 1, 0xFFFFFFFF, np.uint32)
    n2 = C.c_int(-1)
    assert L.rs_debug_rows_list_plan(bits, unit_width, sz, wt, n, max_entries, None, C.byref(n2), launches.ctypes.data,
                                     pre.ctypes.data) == 0 and n2.value == nl.value
    launches = launches[:nl.value].astype(np.int64)
    pres, at = [], 0
    for l in launches:
        pres.append(pre[at: at + int(l[3]) + 1].astype(np.int64))
        at += int(l[3]) + 1
    assert at == n + nl.value and pre[at] == 0xFFFFFFFF  # nothing written past the prefixes
    return 0, limit.value, launches, pres
