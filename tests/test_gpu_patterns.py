"""GPU tests of rs_reconstruct_dev_batch_patterns: a slab of stripes, each with
an erasure pattern of its own, rebuilt in one call.  Every rebuilt row must be,
bit for bit, what the oracle's Reconstruct (a fresh oracle per stripe) puts
there for that stripe's pattern, and no other byte of the slab may change:
present rows, missing rows the call does not rebuild, stripes with nothing to
rebuild and the padding behind every row.
"""
import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5
PAD = 64  # row_stride = S + PAD

# (bits, k, p, sizes)
GEOMS = [
    (16, 128, 32, [64, 192, 4160, 1088]),  # 1088: one bit-sliced tile plus a tail
    (16, 37, 9, [64, 192, 4160]),
    (16, 3, 7, [64, 192, 4160]),
    (16, 2, 1, [64, 192, 4160]),
    (16, 300, 300, [64, 192, 4160]),       # n = 1024 (both rec_half values below)
    (16, 1024, 256, [64, 192]),            # n = 2048
    (16, 2100, 100, [64]),                 # n = 4096
    (8, 10, 4, [64, 192, 4160]),
    (8, 100, 28, [64, 192, 4160]),
    (8, 128, 128, [64, 192, 4160]),
]
CASES = [(b, k, p, S) for b, k, p, sizes in GEOMS for S in sizes]
# P2 twice, P0 in the middle, neighbours with different output counts, not monotonic
PATTERN_OF = [2, 0, 1, 4, 2, 3, 1]


def pattern_table(bits, k, p):
    """[6, k+p] present flags: P0 nothing missing, P1 one data row, P2 p rows
    (data and parity mixed where p >= 2), P3 parity rows only, P4 = P2 shifted
    by one index, and a copy of P2 that no stripe names."""
    rng = np.random.default_rng(bits * 101 + k * 7 + p)
    total = k + p
    t = np.ones((6, total), bool)
    t[1, int(rng.integers(0, k))] = False
    d = int(rng.integers(0, k))
    if p >= 2:
        q = k + int(rng.integers(0, p))
        rest = [i for i in range(total) if i not in (d, q)]
        p2 = np.array(sorted([d, q] + rng.choice(rest, p - 2, replace=False).tolist()))
    else:
        p2 = np.array([d])
    t[2, p2] = False
    t[3, k + rng.choice(p, min(p, 3), replace=False)] = False
    t[4, (p2 + 1) % total] = False
    t[5] = t[2]
    assert (t.sum(axis=1) >= k).all()
    return t


_stripes = {}
_oracle = {}


def stripe(bits, k, p, S, z, tamper=None):
    """Encoded stripe z (k+p rows), computed once and never written; tamper:
    index of a row replaced by other bytes, so the rows are no codeword."""
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


def oracle_rows(bits, k, p, S, z, present, recover_all, tamper=None):
    """{index: row} of the rows a fresh oracle's Reconstruct rebuilds."""
    key = (bits, k, p, S, z, tamper, present.tobytes(), recover_all)
    if key not in _oracle:
        full = stripe(bits, k, p, S, z, tamper)
        lst = [np.array(full[i]) if present[i] else None for i in range(k + p)]
        e, out = orc.Oracle(bits, k, p).reconstruct(lst, recover_all=recover_all)
        assert e == 0, e
        _oracle[key] = {i: out[i] for i in range(k + p) if not present[i] and out[i] is not None}
    return _oracle[key]


def build(bits, k, p, S, table, pattern_of, recover_all, tamper=None, same_data=False):
    """(device slab [ns, k+p, S + PAD] prefilled with FILL, expected numpy array).
    tamper: {stripe: row}.  same_data: every stripe holds stripe 0's bytes."""
    ns, total = len(pattern_of), k + p
    have = np.full((ns, total, S + PAD), FILL, np.uint8)
    exp = np.full((ns, total, S + PAD), FILL, np.uint8)
    for z, q in enumerate(pattern_of):
        present = table[q]
        zz = 0 if same_data else z
        bad = (tamper or {}).get(z)
        full = stripe(bits, k, p, S, zz, bad)
        have[z, present, :S] = full[present]
        exp[z, present, :S] = full[present]
        if not present.all():
            for i, row in oracle_rows(bits, k, p, S, zz, present, recover_all, bad).items():
                exp[z, i, :S] = row
    return torch.from_numpy(have).to(DEV), exp


def run_and_check(c, slab, exp, S, table, pattern_of, recover_all, what, stream=None):
    c.reconstruct_dev_batch_patterns(slab[:, :, :S], table, pattern_of, recover_all, stream=stream)
    torch.cuda.synchronize()
    got = slab.cpu().numpy()
    if not np.array_equal(got, exp):
        z, i = np.argwhere((got != exp).any(axis=2))[0]
        raise AssertionError(f"{what}: stripe {z} (pattern {pattern_of[z]}) row {i} differs")


def check_main(bits, k, p, S, recover_all):
    table = pattern_table(bits, k, p)
    slab, exp = build(bits, k, p, S, table, PATTERN_OF, recover_all)
    if not recover_all:  # the P3 stripe and the parity rows of the P2 / P4 stripes stay as they were
        assert (exp[5, ~table[3], :] == FILL).all()
        for z in (0, 3, 4):
            miss = np.flatnonzero(~table[PATTERN_OF[z]])
            assert (exp[z, miss[miss >= k], :] == FILL).all()
            assert (miss >= k).all() or (exp[z, miss[miss < k], :S] != FILL).any()
    c = rs.ReedSolomon(k, p, bits)
    run_and_check(c, slab, exp, S, table, PATTERN_OF, recover_all, f"{bits} {k}+{p} S={S} all={recover_all}")
    c.close()


@pytest.mark.parametrize("recover_all", [True, False], ids=["all", "data"])
@pytest.mark.parametrize("bits,k,p,S", CASES)
def test_patterns_match_oracle(bits, k, p, S, recover_all):
    check_main(bits, k, p, S, recover_all)


@pytest.mark.parametrize("recover_all", [True, False], ids=["all", "data"])
@pytest.mark.parametrize("S", [64, 192, 4160])
def test_n1024_in_half_tiles(paths, S, recover_all):
    """300+300 with rec_half 1: two 512-thread workgroups per CU."""
    paths("rec_half", 1)
    check_main(16, 300, 300, S, recover_all)


def test_n2048_in_half_tiles(paths):
    paths("rec_half", 1)
    check_main(16, 1024, 256, 192, True)


@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 192), (16, 37, 9, 4160), (8, 10, 4, 192), (8, 128, 128, 4160)])
def test_wide_units(paths, bits, k, p, S):
    """unit_width 0: the 128-byte tile kernels a large grid selects."""
    paths("unit_width", 0)
    check_main(bits, k, p, S, True)


def test_full_field_transforms(paths):
    """sub 0: a 128+32 codec without subfield coordinates."""
    paths("sub", 0)
    check_main(16, 128, 32, 192, True)


@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 1088), (16, 37, 9, 192), (16, 300, 300, 64), (16, 1024, 256, 64),
                                        (8, 10, 4, 192), (8, 100, 28, 192)])
def test_each_stripe_equals_the_one_pattern_batch_call(bits, k, p, S):
    """Stripe by stripe what rs_reconstruct_dev_batch writes for that stripe
    alone with its pattern (reference inversion cache off: the exact locators)."""
    table = pattern_table(bits, k, p)
    slab, _ = build(bits, k, p, S, table, PATTERN_OF, True)
    single = slab.clone()
    c = rs.ReedSolomon(k, p, bits)
    c.reconstruct_dev_batch_patterns(slab[:, :, :S], table, PATTERN_OF)
    c2 = rs.ReedSolomon(k, p, bits)
    c2.set_reference_inversion_cache(False)
    for z, q in enumerate(PATTERN_OF):
        c2.reconstruct_dev_batch(single[z:z + 1, :, :S], table[q])
    torch.cuda.synchronize()
    assert torch.equal(slab, single)
    c.close()
    c2.close()


@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 192), (16, 37, 9, 192), (8, 10, 4, 192), (16, 300, 300, 64)])
def test_an_inconsistent_stripe_follows_the_oracle(bits, k, p, S):
    """Stripe 3 (pattern P4) has one of its present rows tampered: it is rebuilt
    as the oracle rebuilds those rows, and its neighbours are unaffected."""
    table = pattern_table(bits, k, p)
    rows = np.flatnonzero(table[4])
    bad = int(rows[np.random.default_rng(bits + k + p).integers(0, rows.size)])
    slab, exp = build(bits, k, p, S, table, PATTERN_OF, True, tamper={3: bad})
    clean = oracle_rows(bits, k, p, S, 3, table[4], True)
    dirty = oracle_rows(bits, k, p, S, 3, table[4], True, bad)
    assert all(not np.array_equal(clean[i], dirty[i]) for i in clean)  # the tampered row changes what is rebuilt
    c = rs.ReedSolomon(k, p, bits)
    run_and_check(c, slab, exp, S, table, PATTERN_OF, True, f"{bits} {k}+{p} tampered")
    c.close()


def rotation(k, p, ns, shift, lost=(3, 11, 40)):
    total = k + p
    table = np.ones((ns, total), bool)
    for z in range(ns):
        table[z, [(i + z + shift) % total for i in lost]] = False
    return table


def test_rotated_layout_through_the_set_cache():
    """37+9, 46 stripes, stripe z misses shards {3+z, 11+z, 40+z} mod 46: 46
    patterns in one call; the second call finds the set cached.  Then five
    other sets (the cache holds four), and the first one again, rebuilt."""
    bits, k, p, S = 16, 37, 9, 64
    c = rs.ReedSolomon(k, p, bits)
    table = rotation(k, p, 46, 0)
    of = list(range(46))
    for rep in range(2):
        slab, exp = build(bits, k, p, S, table, of, True)
        run_and_check(c, slab, exp, S, table, of, True, f"rotation, call {rep}")
    short = list(range(6))
    for shift in (1, 2, 3, 4, 5, 0):
        t = rotation(k, p, 6, shift)
        slab, exp = build(bits, k, p, S, t, short, True)
        run_and_check(c, slab, exp, S, t, short, True, f"rotation, shift {shift}")
    slab, exp = build(bits, k, p, S, table, of, False)
    run_and_check(c, slab, exp, S, table, of, False, "rotation, data only")
    slab, exp = build(bits, k, p, S, table, of, True)
    run_and_check(c, slab, exp, S, table, of, True, "rotation, after eviction")
    c.close()


@pytest.mark.parametrize("recover_all", [True, False], ids=["all", "data"])
@pytest.mark.parametrize("S", [64, 192, 4160, 1088])
def test_c4_in_the_lds_kernel(paths, S, recover_all):
    """pat_tier 1: 128+32 through the LDS-resident kernel (the main cases run
    it through the bit-sliced decoder, the automatic choice)."""
    paths("pat_tier", 1)
    check_main(16, 128, 32, S, recover_all)


@pytest.mark.parametrize("tier", [1, 2])
def test_c4_with_the_decoder_grid_capped(paths, tier):
    """128+32 x 1088 (two column tiles per stripe) with the bit-sliced decoder's
    persistent grid capped to two workgroups, under each tier that exists."""
    paths("bsdec_grid", 2)
    paths("pat_tier", tier)
    check_main(16, 128, 32, 1088, True)
    check_main(16, 128, 32, 1088, False)


def test_more_stripes_than_one_grid_slice():
    """32768 stripes fill grid.y: the stripes of the second slice must still
    find their own descriptors (and the skipped ones stay untouched)."""
    bits, k, p, S = 16, 3, 7, 64
    ns = 32768 + 5
    table = pattern_table(bits, k, p)
    of = np.zeros(ns, np.int64)
    for z, q in ((0, 1), (1, 2), (32766, 4), (32767, 1), (32768, 2), (32769, 0), (32770, 3), (32772, 4)):
        of[z] = q
    slab, exp = build(bits, k, p, S, table, of.tolist(), True, same_data=True)
    c = rs.ReedSolomon(k, p, bits)
    run_and_check(c, slab, exp, S, table, of, True, "two grid slices")
    c.close()


def test_more_stripes_than_one_launch_takes():
    """A launch takes 2^18 stripes; the call splits the rest off into a second
    stripe range with a pattern set of its own.  Both ranges use P1 and P2, so
    the second must not inherit the first one's descriptor numbers."""
    bits, k, p, S = 16, 2, 1, 64
    ns, total = (1 << 18) + 3, k + p
    table = pattern_table(bits, k, p)
    full = stripe(bits, k, p, S, 0)
    have = np.full((ns, total, S + PAD), FILL, np.uint8)
    have[:, :, :S] = full
    exp = have.copy()
    of = np.zeros(ns, np.int64)
    for z, q in ((0, 2), (5, 1), ((1 << 18) - 1, 2), (1 << 18, 1), ((1 << 18) + 2, 2)):
        of[z] = q
        have[z, ~table[q], :S] = FILL
        exp[z, ~table[q], :S] = FILL
        for i, row in oracle_rows(bits, k, p, S, 0, table[q], True).items():
            exp[z, i, :S] = row
    slab = torch.from_numpy(have).to(DEV)
    c = rs.ReedSolomon(k, p, bits)
    run_and_check(c, slab, exp, S, table, of, True, "two stripe ranges")
    c.close()


@pytest.mark.parametrize("null_stream", [False, True], ids=["side", "null"])
@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 4160), (8, 10, 4, 192)])
def test_stream_order(bits, k, p, S, null_stream):
    """The call is ordered on its stream: behind the copy that brings the rows
    in and ahead of the copy that takes them out, with no host wait between."""
    table = pattern_table(bits, k, p)
    src, exp = build(bits, k, p, S, table, PATTERN_OF, True)
    c = rs.ReedSolomon(k, p, bits)
    slab = torch.zeros_like(src)
    stream = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(3):
            slab.copy_(src, non_blocking=True)
            c.reconstruct_dev_batch_patterns(slab[:, :, :S], table, PATTERN_OF)
            got = slab.clone()
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), exp)
    c.close()
