"""GPU tests that visit every instantiation count of the stream kernel families
(csrc/stream_kernels.hip) against the oracle, bit for bit: every group size
1..8 of the three update calls, every wanted-row count 1..8 of the four direct
decode calls, every (rows 0..6, checks 1..2) of the checked degraded read, and
the syndrome scan in pointer, strided and list form.  Each under both unit widths
(rs_debug_set_path("unit_width", 0 / 1)), the decodes with the direct tier
forced (rows_direct = 1).

Geometries: 10+8 in both fields (ten present rows are two trips of the 4-row
loop and a 2-row tail; eight parity rows allow every count) and GF(2^16) 3+8
(three present rows: the tail loop alone; three data rows: update groups 1..3).
The update and scan tests add GF(2^16) 10+6 and GF(2^8) 10+7, whose parity
rows are one trip and a 2- or 3-row tail of those kernels' loops.
Shard sizes: 64 bytes (almost every lane is past the end) and 8256 (one full
wide GF(2^16) workgroup and a partial second).  Three stripes, a different row
set per stripe where the call takes one.

The references are the oracle's: a stripe is random data plus orc.encode's
parity, so the rows a decode must rebuild are the oracle's rows (the oracle's
own Reconstruct of such a stripe is asserted equal once per geometry), and an
updated or repaired stripe must equal the oracle's encode of its data.  Every
check compares the whole slab, so no other row may change.
"""
import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5
NS = 3
GEOMS = [(16, 10, 8), (8, 10, 8), (16, 3, 8)]
SIZES = [64, 8256]
CASES = [(b, k, p, S, w) for b, k, p in GEOMS for S in SIZES for w in (0, 1)]
IDS = ["gf%d-%d+%d-%dB-width%d" % c for c in CASES]
case_params = pytest.mark.parametrize("bits,k,p,S,width", CASES, ids=IDS)
# the kernels that loop over the parity rows: also parity counts that are no multiple of 4
PARITY_CASES = CASES + [(b, k, p, S, w) for b, k, p in [(16, 10, 6), (8, 10, 7)] for S in SIZES for w in (0, 1)]
parity_case_params = pytest.mark.parametrize("bits,k,p,S,width", PARITY_CASES,
                                             ids=["gf%d-%d+%d-%dB-width%d" % c for c in PARITY_CASES])

_refs = {}


def ref(bits, k, p, S):
    """(old, new) codewords [NS, k+p, S] of a geometry and size: random data and
    the oracle's parity, twice.  Computed once, shared, read-only."""
    key = (bits, k, p, S)
    if key not in _refs:
        rng = np.random.default_rng(bits * 1009 + k * 101 + p * 11 + S)
        pair = []
        for _ in range(2):
            cw = np.empty((NS, k + p, S), np.uint8)
            for z in range(NS):
                cw[z, :k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
                cw[z, k:] = orc.encode(bits, k, p, cw[z, :k])
            cw.setflags(write=False)
            pair.append(cw)
        # the oracle's Reconstruct of such a stripe gives back the stripe's rows
        shards = [np.array(r) for r in pair[0][0]]
        gone = rng.choice(k + p, p, replace=False)
        for i in gone:
            shards[i] = None
        err, out = orc.Oracle(bits, k, p).reconstruct(shards)
        assert err == 0 and all(np.array_equal(out[i], pair[0][0, i]) for i in gone)
        _refs[key] = tuple(pair)
    return _refs[key]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the references are read-only


def same(slab, want, what):
    got = slab.cpu().numpy()
    if not np.array_equal(got, want):
        z, i, c = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError("%s: stripe %d row %d byte %d is %#x, expected %#x" % (what, z, i, c, got[z, i, c], want[z, i, c]))


def row_sets(total, count, seed, among=None):
    """NS different sets of `count` rows out of `among` (default: all rows)."""
    rng = np.random.default_rng(seed)
    pool = np.arange(total) if among is None else np.asarray(among)
    sets = []
    while len(sets) < NS:
        s = sorted(int(i) for i in rng.choice(pool, count, replace=False))
        if s not in sets or count in (0, len(pool)):
            sets.append(s)
    return sets


# ---------------------------------------------------------------- update
def expect_update(bits, k, p, old, new, rows_of):
    """The slab after data rows rows_of[z] of stripe z took the new stripe's
    rows: the oracle's encode of the mixed data."""
    want = np.array(old)
    for z, rows in enumerate(rows_of):
        want[z, rows] = new[z, rows]
        want[z, k:] = orc.encode(bits, k, p, want[z, :k])
    return want


@parity_case_params
def test_update_pointer_form(paths, bits, k, p, S, width):
    """rs_update_dev, one call per stripe, t = 1..min(8, k) changed rows."""
    paths("unit_width", width)
    old, new = ref(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    for t in range(1, min(8, k) + 1):
        rows_of = row_sets(k, t, 100 + t)
        want = expect_update(bits, k, p, old, new, rows_of)
        slab, fresh = dev(old), dev(new)
        for z in range(NS):
            rows = [slab[z, i] if (i >= k or i in rows_of[z]) else None for i in range(k + p)]
            c.update_dev(rows, [fresh[z, j] if j in rows_of[z] else None for j in range(k)])
            for j in rows_of[z]:  # the call writes parity only: the caller stores the new data rows
                slab[z, j] = fresh[z, j]
        torch.cuda.synchronize()
        same(slab, want, "update_dev t=%d" % t)
    c.close()


@parity_case_params
def test_update_batch(paths, bits, k, p, S, width):
    """rs_update_dev_batch, t = 1..min(8, k) changed rows, the same in every stripe."""
    paths("unit_width", width)
    old, new = ref(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    for t in range(1, min(8, k) + 1):
        idx = row_sets(k, t, 200 + t)[0]
        want = expect_update(bits, k, p, old, new, [idx] * NS)
        slab = dev(old)
        c.update_dev_batch(slab, idx, dev(new[:, idx]))
        torch.cuda.synchronize()
        same(slab, want, "update_dev_batch t=%d" % t)
    c.close()


@parity_case_params
def test_update_batch_list(paths, bits, k, p, S, width):
    """rs_update_dev_batch_list, every stripe t = 1..min(8, k) rows of its own:
    one launch of group size t."""
    paths("unit_width", width)
    old, new = ref(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    for t in range(1, min(8, k) + 1):
        rows_of = row_sets(k, t, 300 + t)
        want = expect_update(bits, k, p, old, new, rows_of)
        ent = [(z, j) for z in range(NS) for j in rows_of[z]]
        order = np.random.default_rng(t).permutation(len(ent))
        stripes, idx = [ent[e][0] for e in order], [ent[e][1] for e in order]
        slab = dev(old)
        c.update_dev_batch_list(slab, stripes, idx, dev(np.stack([new[z, j] for z, j in zip(stripes, idx)])))
        torch.cuda.synchronize()
        same(slab, want, "update_dev_batch_list t=%d" % t)
    c.close()


# ---------------------------------------------------------------- direct decode
def holes(cw, erased_of):
    """The slab with rows erased_of[z] of stripe z overwritten."""
    before = np.array(cw)
    for z, rows in enumerate(erased_of):
        before[z, rows] = FILL
    return before


def rebuilt(cw, before, wanted_of):
    want = np.array(before)
    for z, rows in enumerate(wanted_of):
        want[z, rows] = cw[z, rows]
    return want


def flags(total, erased_of, wanted_of):
    pr = np.ones((NS, total), bool)
    rq = np.zeros((NS, total), bool)
    for z in range(NS):
        pr[z, erased_of[z]] = False
        rq[z, wanted_of[z]] = True
    return pr, rq


def decode_case(bits, k, p, S, t, seed):
    """p rows erased per stripe (k present rows), t of them wanted."""
    cw, _ = ref(bits, k, p, S)
    erased_of = row_sets(k + p, p, seed + t)
    wanted_of = [row_sets(k + p, t, seed + 50 + t + z, among=erased_of[z])[0] for z in range(NS)]
    before = holes(cw, erased_of)
    return before, rebuilt(cw, before, wanted_of), flags(k + p, erased_of, wanted_of)


@case_params
def test_rows_pointer_form(paths, bits, k, p, S, width):
    """rs_reconstruct_rows_dev, one call per stripe, t = 1..8 wanted rows."""
    paths("unit_width", width)
    paths("rows_direct", 1)
    c = rs.ReedSolomon(k, p, bits)
    for t in range(1, 9):
        before, want, (pr, rq) = decode_case(bits, k, p, S, t, 400)
        slab = dev(before)
        for z in range(NS):
            c.reconstruct_rows_dev(slab[z], pr[z], rq[z])
        torch.cuda.synchronize()
        same(slab, want, "reconstruct_rows_dev t=%d" % t)
    c.close()


@case_params
def test_rows_batch(paths, bits, k, p, S, width):
    """rs_reconstruct_rows_dev_batch, t = 1..8 wanted rows, one pair for all stripes."""
    paths("unit_width", width)
    paths("rows_direct", 1)
    cw, _ = ref(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    for t in range(1, 9):
        erased = row_sets(k + p, p, 500 + t)[0]
        wanted = row_sets(k + p, t, 550 + t, among=erased)[0]
        before = holes(cw, [erased] * NS)
        want = rebuilt(cw, before, [wanted] * NS)
        pr, rq = flags(k + p, [erased] * NS, [wanted] * NS)
        slab = dev(before)
        c.reconstruct_rows_dev_batch(slab, pr[0], rq[0])
        torch.cuda.synchronize()
        same(slab, want, "reconstruct_rows_dev_batch t=%d" % t)
    c.close()


@case_params
def test_rows_batch_patterns(paths, bits, k, p, S, width):
    """rs_reconstruct_rows_dev_batch_patterns, t = 1..8 wanted rows, a pair per stripe."""
    paths("unit_width", width)
    paths("rows_direct", 1)
    c = rs.ReedSolomon(k, p, bits)
    for t in range(1, 9):
        before, want, (pr, rq) = decode_case(bits, k, p, S, t, 600)
        slab = dev(before)
        c.reconstruct_rows_dev_batch_patterns(slab, pr, rq, list(range(NS)))
        torch.cuda.synchronize()
        same(slab, want, "reconstruct_rows_dev_batch_patterns t=%d" % t)
    c.close()


@case_params
def test_rows_list(paths, bits, k, p, S, width):
    """rs_reconstruct_rows_dev_list, t = 1..8 wanted rows, a pair per stripe."""
    paths("unit_width", width)
    paths("rows_direct", 1)
    c = rs.ReedSolomon(k, p, bits)
    for t in range(1, 9):
        before, want, (pr, rq) = decode_case(bits, k, p, S, t, 700)
        slab = dev(before)
        c.reconstruct_rows_dev_list([slab[z] for z in range(NS)], pr, rq, list(range(NS)))
        torch.cuda.synchronize()
        same(slab, want, "reconstruct_rows_dev_list t=%d" % t)
    c.close()


@case_params
def test_rows_checked(paths, bits, k, p, S, width):
    """rs_reconstruct_rows_checked_dev_batch_patterns, (t, checks) in 0..6 x 1..2:
    k + checks rows present (k + 1 for one check: with 10 + 1 rows two trips
    and a 3-row tail), t of the others wanted, a pair per stripe.  The stripes
    are consistent, so every verdict is OK."""
    paths("unit_width", width)
    paths("rows_direct", 1)
    cw, _ = ref(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    for checks in (1, 2):
        for t in range(0, 7):
            erased_of = row_sets(k + p, p - checks, 800 + 10 * checks + t)
            wanted_of = [row_sets(k + p, t, 850 + t + z, among=erased_of[z])[0] for z in range(NS)]
            before = holes(cw, erased_of)
            want = rebuilt(cw, before, wanted_of)
            pr, rq = flags(k + p, erased_of, wanted_of)
            slab = dev(before)
            verdict = c.reconstruct_rows_checked_dev_batch_patterns(slab, pr, rq, list(range(NS)), checks=checks)
            torch.cuda.synchronize()
            same(slab, want, "checked t=%d checks=%d" % (t, checks))
            assert verdict.tolist() == [rs.ROWS_CHECK_OK] * NS, (t, checks, verdict)
    c.close()


# ---------------------------------------------------------------- syndrome scan
def corrupted(cw, k, S, seed):
    """Stripe 0 with a data shard and stripe 2 with a parity shard changed at
    the first, a middle and the last byte; stripe 1 clean."""
    rng = np.random.default_rng(seed)
    bad = np.array(cw)
    where = {0: int(rng.integers(0, k)), 2: k + int(rng.integers(0, cw.shape[1] - k))}
    for z, i in where.items():
        for col in (0, S // 2 + 1, S - 1):
            bad[z, i, col] ^= int(rng.integers(1, 256))
    return bad, [where[0], rs.SCRUB_CLEAN, where[2]]


@parity_case_params
def test_scan_pointer_form(paths, bits, k, p, S, width):
    """rs_locate_dev with repair, one call per stripe, the rows scattered over a
    pool with no common stride between the parity rows: the scan reads them
    through row pointers.  The pool's other slots must stay as they were."""
    paths("unit_width", width)
    cw, _ = ref(bits, k, p, S)
    bad, verdicts = corrupted(cw, k, S, 900)
    total = k + p
    c = rs.ReedSolomon(k, p, bits)
    for z in range(NS):
        slot = np.random.default_rng(910 + z).permutation(2 * total)[:total]
        assert len(set(np.diff(slot[k:]).tolist())) > 1, "the parity rows would have a common stride"
        pool = np.full((2 * total, S), FILL, np.uint8)
        pool[slot] = bad[z]
        want = np.array(pool)
        want[slot] = cw[z]
        buf = dev(pool)
        got = c.locate_dev([buf[int(i)] for i in slot], repair=True)
        torch.cuda.synchronize()
        assert got == verdicts[z], (z, got)
        same(buf[None], want[None], "locate_dev repair, scattered rows, stripe %d" % z)
    c.close()


@parity_case_params
def test_scan_strided_form(paths, bits, k, p, S, width):
    """rs_locate_dev with repair on a [k+p, S] tensor: equally spaced rows, the
    scan's strided form."""
    paths("unit_width", width)
    cw, _ = ref(bits, k, p, S)
    bad, verdicts = corrupted(cw, k, S, 900)
    c = rs.ReedSolomon(k, p, bits)
    slab = dev(bad)
    got = [c.locate_dev(slab[z], repair=True) for z in range(NS)]
    torch.cuda.synchronize()
    assert got == verdicts
    same(slab, cw, "locate_dev repair")
    c.close()


@parity_case_params
def test_scan_list_form(paths, bits, k, p, S, width):
    """rs_locate_dev_batch with repair, the stripes in another order."""
    paths("unit_width", width)
    cw, _ = ref(bits, k, p, S)
    bad, verdicts = corrupted(cw, k, S, 950)
    c = rs.ReedSolomon(k, p, bits)
    slab = dev(bad)
    order = [2, 0, 1]
    got = c.locate_dev_batch(slab, order, repair=True)
    torch.cuda.synchronize()
    assert got.tolist() == [verdicts[z] for z in order]
    same(slab, cw, "locate_dev_batch repair")
    c.close()
