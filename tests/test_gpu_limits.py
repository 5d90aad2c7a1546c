"""Device rows and stripes 4 GiB and more apart, through every kernel family.

Every case lives in one 6 GiB device buffer that is never initialised: rows of
S = 2240 bytes are views into it, only the rows' own bytes and 64 guard bytes
before and after each are written or read, the guards hold 0xA5 and are checked
after every call together with every row the call must not write.  Two
geometries (tests/limits_cases.py): "far_rows" (the rows of a stripe span more
than 4 GiB; a second stripe sits 1 MiB on, in the gaps) and "far_stripes" (rows
close, the second stripe 4.5 GiB on).  The stripe a case is about is the second
one, so an offset computed in 32 bits anywhere shows as a difference.  The
reference is oracle/orc.py, bit for bit.

No case here sends rows with a data span of 2^32 or more through the encode
(range limits: the known defect of the strided register
kernel); the encodes, verifies, scrubs and the checked rebuild, which encode
fresh parity, run at the far-stripes geometry only.  The batch calls of
reconstruct, selective reconstruct, the checked rebuild and the update list
refuse stripes that interleave, so at far_rows they get the second stripe alone
(batch_of) and the first must come back untouched.
"""
import functools

import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc
from tests import limits_cases as lc

pytestmark = pytest.mark.gpu

S = lc.S_EDGE
G = lc.GUARD
FILL = 0xA5
JUNK = 0x3C  # content of rows a call is to rebuild
CLEAN = rs.SCRUB_CLEAN


class _Holder:
    buf = None


@pytest.fixture(scope="module")
def far():
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory for the 6 GiB row buffer, %.1f GiB free" % (free / 2**30))
    h = _Holder()
    h.buf = torch.empty(lc.BUF_BYTES, dtype=torch.uint8, device="cuda")
    yield h
    torch.cuda.synchronize()
    h.buf = None  # the only reference: later test files must not inherit a cached 6 GiB block
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def codeword(bits, k, p, seed=0, size=S):
    """[k + p, size]: seeded random data rows and the oracle's parity.  Read-only, shared."""
    rng = np.random.default_rng(1000 * k + 7 * p + bits + seed)
    data = rng.integers(0, 256, (k, size), dtype=np.uint8)
    cw = np.concatenate([data, orc.encode(bits, k, p, data)])
    cw.setflags(write=False)
    return cw


def two_stripes(bits, k, p):
    return np.stack([codeword(bits, k, p, 0), codeword(bits, k, p, 1)])


class Rows:
    """Rows of the far buffer at byte offsets offs[...] (any shape), S bytes each."""

    def __init__(self, buf, offs, size=S):
        self.buf, self.offs, self.size = buf, np.asarray(offs, dtype=np.int64), size
        assert self.offs.min() >= G and self.offs.max() + size + G <= buf.numel()
        flat = np.sort(self.offs.reshape(-1))
        assert (np.diff(flat) >= size + 2 * G).all(), "rows and guards must not overlap"

    def view(self, *idx):
        o = int(self.offs[idx])
        return self.buf[o:o + self.size]

    def views(self, *idx):
        return [self.buf[int(o):int(o) + self.size] for o in self.offs[idx]]

    def write(self, vals):
        """vals: uint8 array of shape offs.shape + (size,); the guards are refilled."""
        vals = np.asarray(vals)
        assert vals.shape == self.offs.shape + (self.size,)
        img = np.full((self.offs.size, self.size + 2 * G), FILL, np.uint8)
        img[:, G:G + self.size] = vals.reshape(self.offs.size, self.size)
        dev = torch.from_numpy(img).cuda()
        for j, o in enumerate(self.offs.reshape(-1)):
            self.buf[int(o) - G:int(o) + self.size + G] = dev[j]

    def poke(self, idx, col, xor):
        self.view(*idx)[col] ^= xor

    def check(self, want, what=""):
        """Every row equals `want` and every guard byte is intact."""
        torch.cuda.synchronize()
        got = torch.stack([self.buf[int(o) - G:int(o) + self.size + G] for o in self.offs.reshape(-1)]).cpu().numpy()
        got = got.reshape(self.offs.shape + (self.size + 2 * G,))
        assert (got[..., :G] == FILL).all() and (got[..., G + self.size:] == FILL).all(), "guard bytes written " + what
        rows = got[..., G:G + self.size]
        bad = np.argwhere((rows != np.asarray(want)).any(axis=-1))
        assert bad.size == 0, "%s: rows %s differ" % (what, bad[:8].tolist())


def layout(far, kind, nrows, nst=2, extra=0):
    """(Rows [nst, nrows], slab view [nst, nrows, S]) of a geometry; extra: byte
    offset of the whole layout (the update tests' new rows)."""
    base, rstride, sstride = lc.geometry(kind, nrows)
    base += extra
    offs = base + np.arange(nst, dtype=np.int64)[:, None] * sstride + np.arange(nrows, dtype=np.int64)[None, :] * rstride
    slab = far.buf.as_strided((nst, nrows, S), (sstride, rstride, 1), base)
    assert slab.data_ptr() == far.buf.data_ptr() + base
    return Rows(far.buf, offs), slab


def batch_of(kind, slab):
    """(slab, live, of) for the batch calls that refuse stripes which interleave
    (stripe_stride < (k + p) * row_stride is an argument error): at far_rows, where
    the second stripe lies in the gaps of the first, the call gets the second
    stripe alone, and the first must come back untouched.  live: the stripes
    in the slab; of[z]: the pattern stripe z uses, the later one first."""
    if kind == "far_rows":
        return slab[1:], [1], {1: 1}
    return slab, [0, 1], {0: 1, 1: 0}


def erasures(k, p, seed, count=None):
    rng = np.random.default_rng(seed)
    er = np.sort(rng.choice(k + p, p if count is None else count, replace=False))
    present = np.ones(k + p, bool)
    present[er] = False
    return er, present


def oracle_rebuild(bits, k, p, cw, present):
    """The oracle's reconstruct of every missing row of cw."""
    sh = [np.array(cw[i]) if present[i] else None for i in range(k + p)]
    e, out = orc.Oracle(bits, k, p).reconstruct(sh)
    assert e == 0
    return np.stack(out)


# --------------------------------------------------------------------------- reconstruct
@pytest.mark.parametrize("bits,k,p,tier", lc.REC_CASES)
@pytest.mark.parametrize("kind", lc.GEOMETRIES)
def test_reconstruct_batch(far, paths, kind, bits, k, p, tier):
    """reconstruct_dev_batch (one pattern) and reconstruct_dev_batch_patterns
    (one per stripe, the patterns in the other order), p erasures each: k_rec_bs256
    (strided, and with a descriptor per tile under pat_tier 2), k_rec_lds and
    k_rec_lds_pat (128 + 32 under pat_tier 1)."""
    paths("pat_tier", tier)
    c = rs.ReedSolomon(k, p, bits)
    cw = two_stripes(bits, k, p)
    rows, slab = layout(far, kind, k + p)
    sub, live, of = batch_of(kind, slab)
    pats = [erasures(k, p, 11)[1], erasures(k, p, 12)[1]]
    for z in live:
        assert np.array_equal(oracle_rebuild(bits, k, p, cw[z], pats[of[z]]), cw[z])
    for batch in (False, True):
        cur = np.array(cw)
        for z in live:
            cur[z, ~pats[0 if batch else of[z]]] = JUNK
        rows.write(cur)
        if batch:
            c.reconstruct_dev_batch(sub, pats[0])
        else:
            c.reconstruct_dev_batch_patterns(sub, np.stack(pats), [of[z] for z in live])
        rows.check(cw, "batch" if batch else "patterns")


@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("bits,k,p", lc.ROWS_SHAPES)
@pytest.mark.parametrize("kind", lc.GEOMETRIES)
def test_reconstruct_rows(far, paths, kind, bits, k, p, direct):
    """Selective reconstruct: one wanted row through the direct kernel
    (k_decode_rows with row pointers and strided, k_decode_rows_pat), p wanted
    rows through the reconstruct kernels with a narrowed output set.  Missing
    rows that are not wanted keep their bytes."""
    paths("rows_direct", direct)
    c = rs.ReedSolomon(k, p, bits)
    cw = two_stripes(bits, k, p)
    rows, slab = layout(far, kind, k + p)
    sub, live, of = batch_of(kind, slab)
    ers = [erasures(k, p, 21)[0], erasures(k, p, 22)[0]]
    pres = np.ones((2, k + p), bool)
    req = np.zeros((2, k + p), bool)
    for t in range(2):  # two (present, required) pairs: p rows missing; one of them wanted, or all
        pres[t, ers[t]] = False
        req[t, ers[t][-1 - t] if direct else ers[t]] = True

    def run(what, pair_of, call):
        """pair_of[z]: the pair stripe z is damaged by and rebuilt with (None: left whole)."""
        start, want = np.array(cw), np.array(cw)
        for z, t in enumerate(pair_of):
            if t is not None:
                start[z, ~pres[t]] = JUNK
                want[z, ~pres[t] & ~req[t]] = JUNK
        rows.write(start)
        call()
        rows.check(want, what)

    ptrs = [rows.view(1, i) if pres[1, i] or req[1, i] else None for i in range(k + p)]
    run("rows_dev", [None, 1], lambda: c.reconstruct_rows_dev(ptrs, pres[1], req[1]))
    run("rows_dev_batch", [0 if z in live else None for z in range(2)],
        lambda: c.reconstruct_rows_dev_batch(sub, pres[0], req[0]))
    run("rows_dev_batch_patterns", [of.get(z) for z in range(2)],
        lambda: c.reconstruct_rows_dev_batch_patterns(sub, pres, req, [of[z] for z in live]))


# --------------------------------------------------------------------------- update
def new_data(bits, k, p, idx, seed):
    """(new rows [len(idx), S], the oracle's codeword of the data with them in place) per stripe."""
    rng = np.random.default_rng(seed)
    news, cws = [], []
    for z in range(2):
        nw = rng.integers(0, 256, (len(idx), S), dtype=np.uint8)
        data = np.array(codeword(bits, k, p, z)[:k])
        data[idx] = nw
        news.append(nw)
        cws.append(np.concatenate([data, orc.encode(bits, k, p, data)]))
    return np.stack(news), np.stack(cws)


@pytest.mark.parametrize("bits,k,p", lc.UPDATE_SHAPES)
def test_update_and_encode_idx_row_lists(far, bits, k, p):
    """update_dev and encode_idx_dev over row lists (k_update, pointer form),
    rows and new rows far apart: parity as the oracle encodes the new data."""
    c = rs.ReedSolomon(k, p, bits)
    cw = two_stripes(bits, k, p)
    rows, _ = layout(far, "far_rows", k + p)
    idx = [0, k - 1]
    news, upd = new_data(bits, k, p, idx, 31)
    nrows, _ = layout(far, "far_rows", k + p, extra=2 * lc.MIB)
    rows.write(cw)
    junk = np.full((2, k + p, S), JUNK, np.uint8)
    junk[1, idx] = news[1]
    nrows.write(junk)
    ptrs = [rows.view(1, i) if i in idx or i >= k else None for i in range(k + p)]
    c.update_dev(ptrs, [nrows.view(1, i) if i in idx else None for i in range(k)])
    want = np.array(cw)
    want[1, k:] = upd[1, k:]  # parity moves, the old data rows stay
    rows.check(want, "update_dev")
    nrows.check(junk, "update_dev new rows")
    # encode_idx_dev: every data row once into zeroed parity rows
    z0 = np.array(cw)
    z0[1, k:] = 0
    rows.write(z0)
    for i in range(k):
        c.encode_idx_dev(rows.view(1, i), i, rows.views(1, slice(k, k + p)))
    rows.check(cw, "encode_idx_dev")


@pytest.mark.parametrize("bits,k,p", lc.UPDATE_SHAPES)
@pytest.mark.parametrize("kind", lc.GEOMETRIES)
def test_update_batch(far, kind, bits, k, p):
    """update_dev_batch (k_update, strided form): the new rows lie in the far buffer too."""
    c = rs.ReedSolomon(k, p, bits)
    cw = two_stripes(bits, k, p)
    rows, slab = layout(far, kind, k + p)
    idx = [0, k - 1]
    news, upd = new_data(bits, k, p, idx, 41)
    nrows, nslab = layout(far, kind, k + p, extra=2 * lc.MIB if kind == "far_rows" else 16 * lc.MIB)
    rows.write(cw)
    junk = np.full((2, k + p, S), JUNK, np.uint8)
    junk[:, :2] = news
    nrows.write(junk)
    c.update_dev_batch(slab, idx, nslab[:, :2])
    rows.check(upd, "update_dev_batch")
    nrows.check(junk, "new rows")


@pytest.mark.parametrize("per", [1, 3])
@pytest.mark.parametrize("bits,k,p", lc.UPDATE_SHAPES)
@pytest.mark.parametrize("kind", lc.GEOMETRIES)
def test_update_batch_list(far, kind, bits, k, p, per):
    """update_dev_batch_list (k_update_list): one and three changed rows per
    stripe, rows 0 and k - 1 among them, the second stripe listed first."""
    c = rs.ReedSolomon(k, p, bits)
    cw = two_stripes(bits, k, p)
    rows, slab = layout(far, kind, k + p)
    sub, live, _ = batch_of(kind, slab)
    idx = [k - 1] if per == 1 else [0, k // 2, k - 1]
    idx0 = [0] if per == 1 else idx
    want, ents = np.array(cw), []
    rng = np.random.default_rng(51 + per)
    for z, ix in ((1, idx), (0, idx0)):
        if z not in live:
            continue
        data = np.array(cw[z, :k])
        for i in ix:
            data[i] = rng.integers(0, 256, S, dtype=np.uint8)
            ents.append((z - live[0], i, data[i]))  # stripe numbers count from the slab's first
        want[z] = np.concatenate([data, orc.encode(bits, k, p, data)])
    # the new rows: entry e at row e of a far layout of their own
    base, rstride, _ = lc.geometry(kind, k + p)
    base += 2 * lc.MIB if kind == "far_rows" else 16 * lc.MIB
    noffs = base + np.arange(len(ents), dtype=np.int64) * rstride
    nrows = Rows(far.buf, noffs)
    nslab = far.buf.as_strided((len(ents), S), (rstride, 1), base)
    rows.write(cw)
    nvals = np.stack([e[2] for e in ents])
    nrows.write(nvals)
    c.update_dev_batch_list(sub, [e[0] for e in ents], [e[1] for e in ents], nslab)
    rows.check(want, "update_dev_batch_list")
    nrows.check(nvals, "new rows")


# --------------------------------------------------------------------------- encode and verify
def flips_fail(rows, verify, cells):
    for cell, col in cells:
        rows.poke(cell, col, 0x10)
        assert not verify(), (cell, col)
        rows.poke(cell, col, 0x10)
    assert verify()


@pytest.mark.parametrize("bits,k,p,path", lc.FAR_STRIPE_ENCODES)
def test_encode_verify_far_stripes(far, bits, k, p, path):
    """encode_dev_batch, verify_dev_batch and verify_dev_batch_map over two
    stripes 4.5 GiB apart, one launcher per case."""
    c = rs.ReedSolomon(k, p, bits)
    assert c.encode_path == path
    cw = two_stripes(bits, k, p)
    rows, slab = layout(far, "far_stripes", k + p)
    start = np.array(cw)
    start[:, k:] = FILL
    rows.write(start)
    c.encode_dev_batch(slab)
    rows.check(cw, path)
    flips_fail(rows, lambda: c.verify_dev_batch(slab), [((1, k - 1), S - 1), ((1, k + p - 1), S - 64), ((0, 0), 0)])
    assert not c.verify_dev_batch_map(slab).any()
    rows.poke((1, k), 5, 0x01)
    assert c.verify_dev_batch_map(slab).tolist() == [False, True]
    rows.poke((1, k), 5, 0x01)
    rows.check(cw, "verify wrote")


@pytest.mark.parametrize("bits,k,p,path", lc.GRID_ENCODES)
def test_encode_verify_large_grid(far, bits, k, p, path):
    """65 540 stripes of 64 bytes in one encode_dev_batch / verify_dev_batch:
    more than the 65 535 the grid's y field is documented for, unsliced.
    Columns are independent, so the reference is one oracle call on the
    stripes laid side by side."""
    ns, n = lc.GRID_STRIPES, k + p
    c = rs.ReedSolomon(k, p, bits)
    assert c.encode_path == path
    wide = codeword(bits, k, p, 2, ns * lc.GRID_S)  # [n, ns * 64]
    cw = np.ascontiguousarray(wide.reshape(n, ns, lc.GRID_S).transpose(1, 0, 2))  # [ns, n, 64]
    base = (1 << 32) + G
    whole = Rows(far.buf, [base], ns * n * lc.GRID_S)  # contiguous stripes: guards around the slab
    slab = far.buf.as_strided((ns, n, lc.GRID_S), (n * lc.GRID_S, lc.GRID_S, 1), base)
    start = np.array(cw)
    start[:, k:] = FILL
    whole.write(start.reshape(1, -1))
    c.encode_dev_batch(slab)
    whole.check(cw.reshape(1, -1), path)
    assert c.verify_dev_batch(slab)
    slab[ns - 1, n - 1, 63] ^= 0x80
    assert not c.verify_dev_batch(slab)
    slab[ns - 1, n - 1, 63] ^= 0x80
    slab[ns - 1, 0, 0] ^= 0x01
    assert not c.verify_dev_batch(slab)


# --------------------------------------------------------------------------- scrub and checked rebuild
@pytest.mark.parametrize("batch", [0, 1])
@pytest.mark.parametrize("bits,k,p", lc.SCRUB_SHAPES)
def test_scrub_far_stripes(far, paths, bits, k, p, batch):
    """scrub_dev_batch, locate_dev_batch and scrub_set_dev_batch with repair over
    two stripes 4.5 GiB apart (the verify map, k_syndrome_scan / confirm / fix,
    one stripe at a time and in shared launches): the verdicts are known by
    construction and the slab ends as the oracle's codeword."""
    paths("scrub_batch", batch)
    paths("scrub_chunk", 1 if batch else 0)
    c = rs.ReedSolomon(k, p, bits)
    cw = two_stripes(bits, k, p)
    rows, slab = layout(far, "far_stripes", k + p)
    b0, b1 = k - 1, k + 1
    none = [-1] * rs.LOCATE_SET_MAX
    one = [(b0, 9, 0x10)]
    two = one + [(b1, S - 2, 0x21)]
    # (name, call, damage to stripe 1, verdicts on the clean slab, verdicts on the damaged one)
    calls = [
        ("scrub_dev_batch", lambda: c.scrub_dev_batch(slab, repair=True).tolist(), one, [CLEAN, CLEAN], [CLEAN, b0]),
        ("locate_dev_batch", lambda: c.locate_dev_batch(slab, [1, 0], repair=True).tolist(), one, [CLEAN, CLEAN],
         [b0, CLEAN]),
        ("scrub_set_dev_batch", lambda: [x.tolist() for x in c.scrub_set_dev_batch(slab, repair=True)], two,
         [[0, 0], [none, none]], [[0, 2], [none, [b0, b1] + none[2:]]]),
    ]
    for name, call, damage, clean, verdicts in calls:
        rows.write(cw)
        assert call() == clean, name
        rows.check(cw, name + " clean")
        for i, col, x in damage:
            rows.poke((1, i), col, x)
        assert call() == verdicts, name
        rows.check(cw, name + " repair")


def test_checked_rebuild_far_stripes(far):
    """reconstruct_checked_dev_batch_patterns with repair (k_syndrome_fix_present):
    one erasure in each stripe, one corrupt survivor in the second."""
    bits, k, p = lc.CHECKED_SHAPE
    c = rs.ReedSolomon(k, p, bits)
    cw = two_stripes(bits, k, p)
    rows, slab = layout(far, "far_stripes", k + p)
    checked_case(c, rows, batch_of("far_stripes", slab), cw, k, p)


def checked_case(c, rows, batch, cw, k, p):
    sub, live, of = batch
    gone = [5, k + 2]  # the row each pattern misses
    pats = np.ones((2, k + p), bool)
    pats[0, gone[0]] = pats[1, gone[1]] = False
    cur = np.array(cw)
    for z in live:
        cur[z, gone[of[z]]] = JUNK
    rows.write(cur)
    call = lambda: c.reconstruct_checked_dev_batch_patterns(sub, pats, [of[z] for z in live], repair=True)
    count, shards = call()
    assert count.tolist() == [0] * len(live)
    rows.check(cw, "checked, clean")
    cur[1, k - 2, S - 3] ^= 0x44  # one corrupt survivor in the second stripe
    rows.write(cur)
    count, shards = call()
    assert count.tolist() == [0] * (len(live) - 1) + [1] and shards[-1, 0] == k - 2
    rows.check(cw, "checked, repair")
