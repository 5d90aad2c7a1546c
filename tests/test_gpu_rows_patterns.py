"""GPU tests of rs_reconstruct_rows_dev_batch_patterns: a slab of stripes, each
with a (present, required) pair of its own, rebuilt in one call.  Every wanted
row must be, bit for bit, what the oracle's Reconstruct (a fresh oracle per
stripe) puts there for that stripe's pattern, and no other byte of the slab may
change: present rows, missing rows not asked for, stripes with nothing to
rebuild and the padding behind every row.  The tier is chosen per stripe, so
every case runs under rows_direct -1 (automatic), 0 (restricted transform only)
and 1 (direct kernel for every n <= 2048 stripe).
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

# (bits, k, p, sizes): 64 is one unit per row, 192 no multiple of the wide
# unit's workgroup span, 4160 crosses a workgroup
GEOMS = [
    (16, 128, 32, [64, 192, 1088, 4160]),  # 1088: one bit-sliced tile plus a tail
    (16, 37, 9, [64, 192, 4160]),
    (16, 3, 7, [64, 192, 4160]),
    (16, 2, 1, [64, 192, 4160]),
    (16, 300, 300, [64, 192, 4160]),       # n = 1024
    (16, 1024, 256, [64, 192]),            # n = 2048, at the direct tier's gate
    (16, 2100, 100, [64]),                 # n = 4096, beyond the gate: restricted tier only
    (8, 10, 4, [64, 192, 4160]),
    (8, 100, 28, [64, 192, 4160]),
    (8, 128, 128, [64, 192, 4160]),
]
CASES = [(b, k, p, S) for b, k, p, sizes in GEOMS for S in sizes]
PATTERN_OF = [2, 0, 1, 4, 2, 3, 1]


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
    assert (~pr[3]).sum() == min(p, 3) and (~pr[4]).sum() == n2
    return pr, rq


def test_every_pair_keeps_k_rows_present():
    for bits, k, p, _ in GEOMS:
        pr, _ = pair_tables(bits, k, p)
        assert (pr.sum(axis=1) >= k).all(), (bits, k, p)


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


def build(bits, k, p, S, pr, rq, pattern_of, tamper=None, same_data=False):
    """(device slab [ns, k+p, S + PAD] prefilled with FILL, expected numpy array).
    rq None: every missing row is wanted.  tamper: {stripe: row}.  same_data:
    every stripe holds stripe 0's bytes."""
    ns, total = len(pattern_of), k + p
    have = np.full((ns, total, S + PAD), FILL, np.uint8)
    for z, q in enumerate(pattern_of):
        zz = 0 if same_data else z
        have[z, pr[q], :S] = stripe(bits, k, p, S, zz, (tamper or {}).get(z))[pr[q]]
    exp = have.copy()
    for z, q in enumerate(pattern_of):
        want = ~pr[q] if rq is None else ~pr[q] & rq[q]
        if want.any():
            rows = oracle_rows(bits, k, p, S, 0 if same_data else z, pr[q], (tamper or {}).get(z))
            for i in np.flatnonzero(want):
                exp[z, i, :S] = rows[i]
    return torch.from_numpy(have).to(DEV), exp


def run_and_check(c, slab, exp, S, pr, rq, pattern_of, what, stream=None):
    c.reconstruct_rows_dev_batch_patterns(slab[:, :, :S], pr, rq, pattern_of, stream=stream)
    torch.cuda.synchronize()
    got = slab.cpu().numpy()
    if not np.array_equal(got, exp):
        z, i = np.argwhere((got != exp).any(axis=2))[0]
        raise AssertionError(f"{what}: stripe {z} (pair {pattern_of[z]}) row {i} differs")
    return got


def check_main(bits, k, p, S, knobs=(None,), paths=None, null_required=False):
    pr, rq = pair_tables(bits, k, p)
    if null_required:
        rq = None
    slab0, exp = build(bits, k, p, S, pr, rq, PATTERN_OF)
    # the expectation itself: unwanted missing rows and the padding stay FILL
    assert (exp[:, :, S:] == FILL).all()
    if rq is not None and p >= 3:
        unwanted = ~pr[3] & ~rq[3]
        assert unwanted.any() and (exp[5, unwanted] == FILL).all()
    c = rs.ReedSolomon(k, p, bits)
    for knob in knobs:
        if knob is not None:
            paths("rows_direct", knob)
        run_and_check(c, slab0.clone(), exp, S, pr, rq, PATTERN_OF, f"{bits} {k}+{p} S={S} rows_direct={knob}")
    c.close()


@pytest.mark.parametrize("bits,k,p,S", CASES)
def test_pairs_match_oracle_under_every_tier_choice(paths, bits, k, p, S):
    """rows_direct -1, 0 and 1 each give the oracle's slab, so all three agree."""
    check_main(bits, k, p, S, knobs=(-1, 0, 1), paths=paths)


@pytest.mark.parametrize("bits,k,p,S", CASES)
def test_null_required_is_the_oracles_reconstruct(bits, k, p, S):
    check_main(bits, k, p, S, null_required=True)


SOME = [(16, 128, 32, 1088), (16, 37, 9, 192), (16, 300, 300, 64), (16, 1024, 256, 64), (8, 10, 4, 192), (8, 100, 28, 192)]


@pytest.mark.parametrize("bits,k,p,S", SOME)
def test_each_stripe_equals_the_one_pair_call(bits, k, p, S):
    """Stripe by stripe what rs_reconstruct_rows_dev_batch writes for that stripe alone with its pair."""
    pr, rq = pair_tables(bits, k, p)
    slab, _ = build(bits, k, p, S, pr, rq, PATTERN_OF)
    single = slab.clone()
    c = rs.ReedSolomon(k, p, bits)
    c.reconstruct_rows_dev_batch_patterns(slab[:, :, :S], pr, rq, PATTERN_OF)
    c2 = rs.ReedSolomon(k, p, bits)
    for z, q in enumerate(PATTERN_OF):
        c2.reconstruct_rows_dev_batch(single[z:z + 1, :, :S], pr[q], rq[q])
    torch.cuda.synchronize()
    assert torch.equal(slab, single)
    c.close()
    c2.close()


@pytest.mark.parametrize("bits,k,p,S", SOME)
def test_null_required_equals_the_patterns_call(bits, k, p, S):
    """required=None on one slab, rs_reconstruct_dev_batch_patterns(recover_all=1) on its twin."""
    pr, _ = pair_tables(bits, k, p)
    slab, _ = build(bits, k, p, S, pr, None, PATTERN_OF)
    twin = slab.clone()
    c = rs.ReedSolomon(k, p, bits)
    c.reconstruct_rows_dev_batch_patterns(slab[:, :, :S], pr, None, PATTERN_OF)
    c2 = rs.ReedSolomon(k, p, bits)
    c2.reconstruct_dev_batch_patterns(twin[:, :, :S], pr, PATTERN_OF, True)
    torch.cuda.synchronize()
    assert torch.equal(slab, twin)
    c.close()
    c2.close()


@pytest.mark.parametrize("knob", [-1, 0, 1])
@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 192), (16, 37, 9, 192), (8, 10, 4, 192), (16, 300, 300, 64)])
def test_an_inconsistent_stripe_follows_the_oracle(paths, bits, k, p, S, knob):
    """Stripe 3 (pair P4) has one of its present rows tampered: its wanted rows
    are the oracle's for those rows, each differs from the clean case, and the
    neighbours are unaffected."""
    paths("rows_direct", knob)
    pr, rq = pair_tables(bits, k, p)
    rows = np.flatnonzero(pr[4])
    bad = int(rows[np.random.default_rng(bits + k + p).integers(0, rows.size)])
    slab, exp = build(bits, k, p, S, pr, rq, PATTERN_OF, tamper={3: bad})
    clean = oracle_rows(bits, k, p, S, 3, pr[4])
    dirty = oracle_rows(bits, k, p, S, 3, pr[4], bad)
    wanted = np.flatnonzero(~pr[4] & rq[4])
    assert wanted.size and all(not np.array_equal(clean[i], dirty[i]) for i in wanted)
    c = rs.ReedSolomon(k, p, bits)
    run_and_check(c, slab, exp, S, pr, rq, PATTERN_OF, f"{bits} {k}+{p} tampered, rows_direct={knob}")
    c.close()


@pytest.mark.parametrize("width", [0, 1], ids=["wide", "narrow"])
@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 192), (16, 37, 9, 4160), (16, 1024, 256, 64), (8, 10, 4, 192),
                                        (8, 128, 128, 4160)])
def test_unit_widths(paths, bits, k, p, S, width):
    """unit_width 0: the 32-byte (GF(2^8): 16-byte) units a large grid selects; 1: the narrow ones."""
    paths("unit_width", width)
    check_main(bits, k, p, S, knobs=(-1, 1), paths=paths)


@pytest.mark.parametrize("tier", [1, 2])
@pytest.mark.parametrize("S", [192, 1088])
def test_c4_restricted_stripes_under_each_pattern_tier(paths, S, tier):
    """128+32: the restricted stripes through the LDS-resident kernel (1) and the bit-sliced decoder (2)."""
    paths("pat_tier", tier)
    check_main(16, 128, 32, S, knobs=(-1, 0), paths=paths)


@pytest.mark.parametrize("half", [0, 1])
def test_n1024_with_both_tile_shapes(paths, half):
    paths("rec_half", half)
    check_main(16, 300, 300, 192, knobs=(-1, 0), paths=paths)


def test_mixed_row_counts_in_one_call(paths):
    """40+40 at S = 64 under rows_direct 1: stripes with t = 1, 2, 3, 5, 8 and
    11 wanted rows, so five values of NT run as launch groups of their own and
    the t = 11 stripe joins two more (6 + 5)."""
    bits, k, p, S = 16, 40, 40, 64
    total = k + p
    counts = [3, 1, 8, 11, 2, 5, 1, 8]
    rng = np.random.default_rng(4040)
    pr = np.ones((len(counts), total), bool)
    rq = np.zeros((len(counts), total), bool)
    for q, t in enumerate(counts):
        miss = np.sort(rng.choice(total, min(t + 4, p), replace=False))
        pr[q, miss] = False
        rq[q, rng.choice(miss, t, replace=False)] = True
    assert (pr.sum(axis=1) >= k).all() and ((~pr & rq).sum(axis=1) == counts).all()
    of = list(range(len(counts)))
    slab, exp = build(bits, k, p, S, pr, rq, of)
    c = rs.ReedSolomon(k, p, bits)
    for knob in (1, -1):
        paths("rows_direct", knob)
        run_and_check(c, slab.clone(), exp, S, pr, rq, of, f"mixed t, rows_direct={knob}")
    c.close()


def rotation(k, p, ns, shift):
    """Stripe z misses shard (z + shift) mod (k+p) and wants it."""
    total = k + p
    pr = np.ones((ns, total), bool)
    for z in range(ns):
        pr[z, (z + shift) % total] = False
    return pr, np.ones((ns, total), bool)


def test_rotated_layout_through_the_set_cache():
    """37+9, 46 stripes, stripe z misses shard z: 46 one-erasure pairs, one
    launch; the second call finds the set cached.  Then five other sets (the
    cache holds four) on a side stream with nothing synchronised in between, so
    sets are evicted while earlier launches may still be queued, and the first
    set again, rebuilt."""
    bits, k, p, S = 16, 37, 9, 64
    c = rs.ReedSolomon(k, p, bits)
    pr, rq = rotation(k, p, 46, 0)
    of = list(range(46))
    for rep in range(2):
        slab, exp = build(bits, k, p, S, pr, rq, of)
        run_and_check(c, slab, exp, S, pr, rq, of, f"rotation, call {rep}")
    short = list(range(6))
    jobs = []
    for shift in (1, 2, 3, 4, 5, 7):
        t = rotation(k, p, 6, shift)
        jobs.append((t,) + build(bits, k, p, S, t[0], t[1], short))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for (tp, tr), slab, _ in jobs:
            c.reconstruct_rows_dev_batch_patterns(slab[:, :, :S], tp, tr, short)
    torch.cuda.synchronize()
    for n, (_, slab, exp) in enumerate(jobs):
        assert np.array_equal(slab.cpu().numpy(), exp), f"rotation, queued call {n}"
    slab, exp = build(bits, k, p, S, pr, rq, of)
    run_and_check(c, slab, exp, S, pr, rq, of, "rotation, after eviction")
    c.close()


def test_a_list_longer_than_two_grid_slices():
    """65539 stripes of 2+1 at S = 64, every stripe with one missing row (shard
    z mod 3): one launch group whose list splits across grid.y slices.  Stripes
    0, 65534, 65535, 65536 and 65538 hold data of their own and are checked
    against the oracle; the others hold stripe 0's bytes, are checked against
    the oracle's rows for those and, stripe by stripe, against a second call."""
    bits, k, p, S = 16, 2, 1, 64
    ns, total = 65539, k + p
    own = (0, 65534, 65535, 65536, 65538)
    pr = ~np.eye(3, dtype=bool)
    rq = np.ones((3, total), bool)
    of = np.arange(ns) % 3
    have = np.full((ns, total, S + PAD), FILL, np.uint8)
    full = stripe(bits, k, p, S, 0)
    for q in range(3):
        have[q::3, pr[q], :S] = full[pr[q]]
    for z in own:
        have[z, pr[of[z]], :S] = stripe(bits, k, p, S, z)[pr[of[z]]]
    exp = have.copy()
    for q in range(3):
        exp[q::3, q, :S] = oracle_rows(bits, k, p, S, 0, pr[q])[q]
    for z in own:
        exp[z, of[z], :S] = oracle_rows(bits, k, p, S, z, pr[of[z]])[int(of[z])]
    slab = torch.from_numpy(have).to(DEV)
    twin = slab.clone()
    c = rs.ReedSolomon(k, p, bits)
    got = run_and_check(c, slab, exp, S, pr, rq, of, "long list")
    for z in own:
        assert np.array_equal(got[z], exp[z]), z
    c.reconstruct_rows_dev_batch_patterns(twin[:, :, :S], pr, rq, of)
    torch.cuda.synchronize()
    assert torch.equal(slab, twin)
    c.close()


@pytest.mark.parametrize("null_stream", [False, True], ids=["side", "null"])
@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 4160), (8, 10, 4, 192)])
def test_stream_order(bits, k, p, S, null_stream):
    """The call is ordered on its stream: behind the kernel that brings the
    rows in and ahead of the one that takes them out, with no host wait between."""
    pr, rq = pair_tables(bits, k, p)
    src, exp = build(bits, k, p, S, pr, rq, PATTERN_OF)
    c = rs.ReedSolomon(k, p, bits)
    slab = torch.zeros_like(src)
    stream = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(3):
            slab.copy_(src, non_blocking=True)
            c.reconstruct_rows_dev_batch_patterns(slab[:, :, :S], pr, rq, PATTERN_OF)
            got = slab.clone()
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), exp)
    c.close()
