"""GPU tests of the checked degraded read
(rs_reconstruct_rows_checked_dev_batch_patterns): the writes are
those of rs_reconstruct_rows_dev_batch_patterns, bit for bit and whatever the
verdict (the oracle's Reconstruct of the rows marked present, a fresh oracle
per stripe; no other byte of the slab changes), and the verdict of a stripe
says whether the rows marked present are consistent.  Slabs as in
tests/test_gpu_rows_patterns.py: seven stripes over a pattern table, row
stride S + 64, 0xA5 in everything that is not a present row.  Every case runs
under rows_direct -1, 0 and 1 and with checks 1 and 2.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import leopard_np, orc
from reedsolomon16_amd import _capi
from tests import limits_cases as lc
from tests.scrub_set_util import gf_mul
from tests.test_gpu_rows_patterns import DEV, FILL, PAD, stripe

pytestmark = pytest.mark.gpu

OK, BAD, NONE = rs.ROWS_CHECK_OK, rs.ROWS_CHECK_BAD, rs.ROWS_CHECK_NONE
KNOBS = (-1, 0, 1)
CHECKS = (1, 2)

# (bits, k, p, sizes) of tests/test_gpu_rows_patterns.py, less its 1088
GEOMS = [
    (16, 128, 32, [64, 192, 4160]),
    (16, 37, 9, [64, 192, 4160]),
    (16, 3, 7, [64, 192, 4160]),
    (16, 2, 1, [64, 192, 4160]),
    (16, 300, 300, [64, 192, 4160]),
    (16, 1024, 256, [64, 192]),   # n = 2048, at the direct tier's gate
    (16, 2100, 100, [64]),        # n = 4096: the check-only form plus the restricted tier
    (8, 10, 4, [64, 192, 4160]),
    (8, 100, 28, [64, 192, 4160]),
    (8, 128, 128, [64, 192, 4160]),
]
CASES = [(b, k, p, S) for b, k, p, sizes in GEOMS for S in sizes]
WITH_TWO = [(b, k, p, S) for b, k, p, S in CASES if p >= 3]  # geometries with a pattern of c_z = 2


def tables(bits, k, p):
    """([npat, k+p] present, required, pattern_of[7]).  P0 nothing missing; P1
    one data row missing and wanted; and where p >= 3: P2 min(p - 2, 7) rows
    missing, data and parity mixed, all wanted; P3 exactly k + 2 rows marked
    present, one of the others (a data row) wanted; P4 a data and a parity row
    missing, the data row wanted."""
    rng = np.random.default_rng(bits * 211 + k * 5 + p)
    total = k + p
    npat = 5 if p >= 3 else 2
    pr = np.ones((npat, total), bool)
    rq = np.zeros((npat, total), bool)
    rq[0] = True
    pr[1, int(rng.integers(0, k))] = False
    rq[1] = True
    if p < 3:
        return pr, rq, [1, 0, 1, 0, 0, 1, 1]
    n2 = min(p - 2, 7)
    d, q = int(rng.integers(0, k)), k + int(rng.integers(0, p))
    rest = [i for i in range(total) if i not in (d, q)]
    p2 = [d, q][:n2] + rng.choice(rest, max(n2 - 2, 0), replace=False).tolist()
    pr[2, p2] = False
    rq[2] = True
    out = np.sort(rng.choice(total, p - 2, replace=False)) if p > 2 else []
    if not (np.asarray(out) < k).any():
        out[0] = int(rng.integers(0, k))
    pr[3, out] = False
    rq[3, int(np.flatnonzero(~pr[3])[0])] = True
    pr[4, [int(rng.integers(0, k)), k + int(rng.integers(0, p))]] = False
    rq[4, :k] = True
    return pr, rq, [2, 0, 1, 3, 4, 1, 3]


def cz_of(pr, k, checks):
    return np.minimum(checks, pr.sum(axis=1) - k)


# the stripes a test tampers with, by what serves them under the automatic knob
FUSED_Z, REST_Z, ONLY_Z = 2, 0, 1  # pattern P1; P2 (p >= 3); P0, the check-only form


def test_checks_per_pattern():
    """c_z of every (geometry, pattern), and what keeps the tests below from
    passing vacuously: every tampered stripe is checked."""
    for bits, k, p, _ in GEOMS:
        pr, rq, of = tables(bits, k, p)
        want = ~pr & rq
        assert (pr.sum(axis=1) >= k).all() and len(of) == 7 and set(of) == set(range(len(pr)))
        assert want[0].sum() == 0 and want[1].sum() == 1 and not pr[1, :k].all()
        for checks in CHECKS:
            cz = cz_of(pr, k, checks)
            if p >= 3:
                assert (cz == checks).all(), (bits, k, p)
                assert want[2].sum() == min(p - 2, 7) == (~pr[2]).sum()
                assert pr[3].sum() == k + 2 and want[3].sum() == 1 and (~pr[3] & ~want[3]).sum() == p - 3
                assert want[4].sum() == 1 and (~pr[4]).sum() == 2
                assert cz[of[FUSED_Z]] >= 1 and cz[of[REST_Z]] >= 1 and cz[of[ONLY_Z]] >= 1
                assert (of[FUSED_Z], of[REST_Z], of[ONLY_Z]) == (1, 2, 0)
            else:
                # 2+1: the one checked case is the pattern with nothing missing
                assert (bits, k, p) == (16, 2, 1) and cz.tolist() == [1, 0]
                assert of[ONLY_Z] == 0 and of[FUSED_Z] == 1


def tampered(bits, k, p, S, z, tamper):
    """Stripe z with tamper = {row: {col: xor}} applied (tamper None: clean)."""
    full = stripe(bits, k, p, S, z)
    if not tamper:
        return full
    full = np.array(full)
    for row, cols in tamper.items():
        for col, x in cols.items():
            full[row, col] ^= x
    return full


def oracle_rows(bits, k, p, full, present):
    lst = [np.array(full[i]) if present[i] else None for i in range(k + p)]
    e, out = orc.Oracle(bits, k, p).reconstruct(lst, recover_all=True)
    assert e == 0, e
    return out


def build(bits, k, p, S, pr, rq, of, tamper=None, garbage=False):
    """(device slab [7, k+p, S + PAD], expected numpy array).  tamper: {stripe:
    {row: {col: xor}}}.  garbage: rows not marked present hold seeded random
    bytes instead of FILL."""
    ns, total = len(of), k + p
    have = np.full((ns, total, S + PAD), FILL, np.uint8)
    if garbage:
        have[:, :, :S] = np.random.default_rng(S + k).integers(0, 256, (ns, total, S), dtype=np.uint8)
    fulls = []
    for z, q in enumerate(of):
        fulls.append(tampered(bits, k, p, S, z, (tamper or {}).get(z)))
        have[z, pr[q], :S] = fulls[z][pr[q]]
    exp = have.copy()
    for z, q in enumerate(of):
        want = ~pr[q] & rq[q]
        if want.any():
            rows = oracle_rows(bits, k, p, fulls[z], pr[q])
            for i in np.flatnonzero(want):
                exp[z, i, :S] = rows[i]
    return torch.from_numpy(have).to(DEV), exp


def run(c, slab, exp, S, pr, rq, of, checks, what):
    v = c.reconstruct_rows_checked_dev_batch_patterns(slab[:, :, :S], pr, rq, of, checks=checks)
    torch.cuda.synchronize()
    got = slab.cpu().numpy()
    if not np.array_equal(got, exp):
        z, i = np.argwhere((got != exp).any(axis=2))[0]
        raise AssertionError(f"{what}: stripe {z} (pattern {of[z]}) row {i} differs")
    return v.tolist()


def every_route(paths, bits, k, p, S, pr, rq, of, slab0, exp, verdict_of, what):
    """The call under every knob and check count on copies of slab0: the slab
    ends as exp and the verdicts are verdict_of(checks)."""
    c = rs.ReedSolomon(k, p, bits)
    for knob in KNOBS:
        paths("rows_direct", knob)
        for checks in CHECKS:
            w = f"{bits} {k}+{p} S={S} {what} rows_direct={knob} checks={checks}"
            assert run(c, slab0.clone(), exp, S, pr, rq, of, checks, w) == verdict_of(checks), w
    c.close()


def clean_verdicts(pr, k, of, checks):
    cz = cz_of(pr, k, checks)
    return [OK if cz[q] else NONE for q in of]


@pytest.mark.parametrize("bits,k,p,S", CASES)
def test_clean_slab(paths, bits, k, p, S):
    pr, rq, of = tables(bits, k, p)
    slab0, exp = build(bits, k, p, S, pr, rq, of)
    assert (exp[:, :, S:] == FILL).all()
    every_route(paths, bits, k, p, S, pr, rq, of, slab0, exp, lambda ch: clean_verdicts(pr, k, of, ch), "clean")
    # the unchecked call writes the same bytes; nbad is 0; checks = 0 checks nothing
    c = rs.ReedSolomon(k, p, bits)
    twin = slab0.clone()
    c.reconstruct_rows_dev_batch_patterns(twin[:, :, :S], pr, rq, of)
    torch.cuda.synchronize()
    assert np.array_equal(twin.cpu().numpy(), exp)
    assert run(c, slab0.clone(), exp, S, pr, rq, of, 0, "checks=0") == [NONE] * len(of)
    nbad, verdict = C.c_int(5), np.full(len(of), 9, np.int32)
    slab = slab0.clone()
    tab, req = pr.astype(np.uint8), rq.astype(np.uint8)
    ofa = np.asarray(of, np.uint32)
    assert c._L.rs_reconstruct_rows_checked_dev_batch_patterns(
        c._h, slab.data_ptr(), slab.stride(1), slab.stride(0), len(of), tab.ctypes.data_as(C.POINTER(C.c_uint8)),
        req.ctypes.data_as(C.POINTER(C.c_uint8)), len(tab), ofa.ctypes.data_as(C.POINTER(C.c_uint32)), S, 2,
        verdict.ctypes.data, C.byref(nbad), None) == 0
    assert nbad.value == 0 and verdict.tolist() == clean_verdicts(pr, k, of, 2)
    assert np.array_equal(slab.cpu().numpy(), exp)
    c.close()


def symbol_cols(bits, S):
    """{name: byte column} of the tampered byte: the first unit, a unit of the
    second workgroup at S = 4160 (narrow units: 256 of them cover 4096 bytes of
    a GF(2^16) row, 2048 of a GF(2^8) row), the last unit; GF(2^16): low bytes,
    and high bytes (32 above the symbol's low byte) in two more cases."""
    cols = {"first": 0, "last": S - 1 if bits == 8 else S - 33}
    if bits == 16:
        cols["first-high"] = 32
        cols["last-high"] = S - 1
    if S == 4160:
        cols["second-wg"] = 4096 + 8 if bits == 16 else 2048 + 8
    return cols


def pick_present(pr_row, seed):
    rows = np.flatnonzero(pr_row)
    return int(rows[np.random.default_rng(seed).integers(0, rows.size)])


@pytest.mark.parametrize("bits,k,p,S", CASES)
def test_one_tampered_symbol_per_tier(paths, bits, k, p, S):
    """One byte of one survivor changed in the P1 stripe (fused under the
    automatic knob) and, where p >= 3, in the P2 stripe (the unchecked route
    plus a check-only entry): exactly those stripes are BAD, their wanted rows
    are the oracle's Reconstruct of the tampered stripe, nothing else changes.
    2+1: its P1 stripes have no redundancy left (NONE), so the tampered stripe
    that must be BAD is the P0 one."""
    pr, rq, of = tables(bits, k, p)
    zs = [FUSED_Z, REST_Z] if p >= 3 else [FUSED_Z, ONLY_Z]
    for name, col in symbol_cols(bits, S).items():
        tamper = {z: {pick_present(pr[of[z]], col + z): {col: 0x5A}} for z in zs}
        slab0, exp = build(bits, k, p, S, pr, rq, of, tamper)

        def verdicts(checks):
            cz = cz_of(pr, k, checks)
            return [NONE if not cz[q] else BAD if z in zs else OK for z, q in enumerate(of)]

        assert all(BAD in verdicts(ch) for ch in CHECKS)
        every_route(paths, bits, k, p, S, pr, rq, of, slab0, exp, verdicts, "tampered " + name)


def to_cols(bits, q):
    """Byte columns (low, high or None) of symbol q of a row."""
    return (q, None) if bits == 8 else (q // 32 * 64 + q % 32, q // 32 * 64 + q % 32 + 32)


def check_weights(bits, k, p, present, l):
    out = np.zeros(k + p, np.uint32)
    pr8 = np.ascontiguousarray(present, np.uint8)
    assert _capi.lib().rs_debug_check_weights(bits, k, p, pr8.ctypes.data_as(C.POINTER(C.c_uint8)), l, out.ctypes.data) == 0
    return out.astype(np.int64)


@pytest.mark.parametrize("bits,k,p,S", WITH_TWO)
def test_adversarial_pair(paths, bits, k, p, S):
    """Two survivors changed at one symbol so that check 0 cancels (D_b = D_a *
    h_0[a] / h_0[b]): OK with one check, the boundary the header states, and BAD
    with two, so check 1 is no copy of check 0.  In the P1 stripe (fused), the
    P0 stripe (check-only) and the P3 stripe (k + 2 rows marked present)."""
    pr, rq, of = tables(bits, k, p)
    F = leopard_np.field(bits)
    zs = [FUSED_Z, ONLY_Z, 3]
    assert of[3] == 3
    nsym = S if bits == 8 else S // 2
    tamper = {}
    for z in zs:
        rng = np.random.default_rng(z + S + p)
        rows = np.flatnonzero(pr[of[z]])
        a, b = (int(x) for x in rng.choice(rows, 2, replace=False))
        h0 = check_weights(bits, k, p, pr[of[z]], 0)
        Da = int(rng.integers(1, 1 << bits))
        inv_b = int(F._exp[F.sub_mod(0, F._log[h0[b]])])
        Db = int(gf_mul(bits, gf_mul(bits, Da, h0[a]), inv_b))
        lo, hi = to_cols(bits, int(rng.integers(0, nsym)))
        tamper[z] = {a: {lo: Da & 255}, b: {lo: Db & 255}}
        if hi is not None:
            tamper[z][a][hi] = Da >> 8
            tamper[z][b][hi] = Db >> 8
    slab0, exp = build(bits, k, p, S, pr, rq, of, tamper)
    clean = build(bits, k, p, S, pr, rq, of)[1]
    assert not np.array_equal(exp[FUSED_Z], clean[FUSED_Z]), "the pair reaches the rebuilt row"
    every_route(paths, bits, k, p, S, pr, rq, of, slab0, exp,
                lambda ch: [BAD if ch == 2 and z in zs else OK for z in range(len(of))], "adversarial pair")


@pytest.mark.parametrize("bits,k,p,S", CASES)
def test_rows_not_marked_present_are_never_read(paths, bits, k, p, S):
    """Random bytes in every row that is not marked present: the missing row
    that is not wanted (P4), the rows that exist but are not marked (P3) and the
    rows about to be rebuilt.  Rows and verdicts are those of the clean slab."""
    pr, rq, of = tables(bits, k, p)
    slab0, exp = build(bits, k, p, S, pr, rq, of, garbage=True)
    ref = build(bits, k, p, S, pr, rq, of)[1]
    for z, q in enumerate(of):
        want = ~pr[q] & rq[q]
        assert np.array_equal(exp[z, want], ref[z, want]) and np.array_equal(exp[z, pr[q]], ref[z, pr[q]])
        if p >= 3 and q in (3, 4):
            assert (exp[z, ~pr[q] & ~want, :S] != FILL).any()
    every_route(paths, bits, k, p, S, pr, rq, of, slab0, exp, lambda ch: clean_verdicts(pr, k, of, ch), "garbage")


@pytest.mark.parametrize("bits,k,p,S", CASES)
def test_check_only(paths, bits, k, p, S):
    """A stripe with nothing missing and one tampered row: BAD, nothing written."""
    pr, rq, of = tables(bits, k, p)
    col = symbol_cols(bits, S)["last"]
    tamper = {ONLY_Z: {pick_present(pr[0], S + p): {col: 0x21}}}
    slab0, exp = build(bits, k, p, S, pr, rq, of, tamper)

    def verdicts(checks):
        cz = cz_of(pr, k, checks)
        return [NONE if not cz[q] else BAD if z == ONLY_Z else OK for z, q in enumerate(of)]

    every_route(paths, bits, k, p, S, pr, rq, of, slab0, exp, verdicts, "check-only")
    # a slab of such stripes alone: no row is wanted anywhere
    c = rs.ReedSolomon(k, p, bits)
    only = slab0[ONLY_Z:ONLY_Z + 1].clone()
    v = c.reconstruct_rows_checked_dev_batch_patterns(only[:, :, :S], pr[:1], None, [0], checks=1)
    assert v.tolist() == [BAD] and torch.equal(only, slab0[ONLY_Z:ONLY_Z + 1])
    c.close()


@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 192), (8, 100, 28, 192)])
def test_hand_over_to_the_checked_rebuild(bits, k, p, S):
    """The BAD stripes of the tampered slab go to
    reconstruct_checked_dev_batch_patterns(repair=True): it names the tampered
    survivor and the stripe ends as the codeword."""
    pr, rq, of = tables(bits, k, p)
    zs = [FUSED_Z, REST_Z, 3]
    rows = {z: pick_present(pr[of[z]], 7 * z + 1) for z in zs}
    slab, exp = build(bits, k, p, S, pr, rq, of, {z: {rows[z]: {S - 1: 0x5A}} for z in zs})
    c = rs.ReedSolomon(k, p, bits)
    v = run(c, slab, exp, S, pr, rq, of, 2, "hand-over")
    assert [z for z, x in enumerate(v) if x == BAD] == sorted(zs)
    for z in zs:
        count, shards = c.reconstruct_checked_dev_batch_patterns(slab[z:z + 1, :, :S], pr[of[z]][None], [0], repair=True)
        assert count.tolist() == [1] and shards[0, 0] == rows[z], (z, count, shards)
        assert np.array_equal(slab[z, :, :S].cpu().numpy(), stripe(bits, k, p, S, z))
    assert (slab[:, :, S:] == FILL).all()
    c.close()


# ---------------------------------------------------------------- rows and stripes 4 GiB apart
from tests.test_gpu_limits import JUNK, batch_of, far, layout, two_stripes  # noqa: E402,F401


@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("bits,k,p", lc.ROWS_SHAPES)
@pytest.mark.parametrize("kind", lc.GEOMETRIES)
def test_far_apart(far, paths, kind, bits, k, p, direct):
    """tests/test_gpu_limits.py::test_reconstruct_rows' layouts: one missing
    row wanted (the fused kernel under direct = 1, the reconstruct kernels plus
    the check-only form under 0), the stripe this is about tampered in its
    last symbol and then clean; at far_stripes the other stripe is the
    opposite."""
    paths("rows_direct", direct)
    c = rs.ReedSolomon(k, p, bits)
    cw = two_stripes(bits, k, p)
    rows, slab = layout(far, kind, k + p)
    sub, live, of = batch_of(kind, slab)
    pres = np.ones((2, k + p), bool)
    pres[0, 3], pres[1, k + 1] = False, False
    req = np.ones((2, k + p), bool)
    for dirty in (1, 0):  # the stripe whose survivor k - 1 is tampered
        start = np.array(cw)
        start[dirty, k - 1, lc.S_EDGE - 1] ^= 0x5A
        want = np.array(start)
        for z in live:
            miss = int(np.flatnonzero(~pres[of[z]])[0])
            want[z, miss] = oracle_rows(bits, k, p, start[z], pres[of[z]])[miss]
            start[z, miss] = JUNK
        rows.write(start)
        v = c.reconstruct_rows_checked_dev_batch_patterns(sub, pres, req, [of[z] for z in live], checks=2)
        rows.check(want, f"{kind} dirty={dirty}")
        assert v.tolist() == [BAD if z == dirty else OK for z in live]
    c.close()
