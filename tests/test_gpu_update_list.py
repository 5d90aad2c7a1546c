"""GPU tests of the batched update from a list of changed rows, a different set
per stripe (rs_update_dev_batch_list; stream_kernels.hip k_update_list) against the
oracle: afterwards every named stripe must be, bit for bit, the new data and
the oracle's encode of it, and nothing else may have been written.
"""
import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS, PAD = 8, 64
GEOMS = [(16, 128, 32), (16, 37, 9), (16, 3, 7), (16, 2, 1), (16, 300, 300), (8, 10, 4), (8, 100, 28), (8, 128, 128)]
# 64: one unit per row; 192: no multiple of a wide unit's workgroup span; 4160: crosses a workgroup
SIZES = [64, 192, 4096 + 64]


def changed_rows(k, seed):
    """The changed data indices per stripe: none, 1, the same 1 (a shared table),
    3 with 0 and k-1, 9 (5 + 4), 16 (8 + 8 in two rounds), all k rows where
    k <= 37 else 2, none; every count capped at k."""
    rng = np.random.default_rng(seed)

    def pick(t, must=()):
        t = min(t, k)
        rest = [j for j in rng.permutation(k) if j not in must]
        return sorted(int(j) for j in (list(must) + rest)[:t])

    one = pick(1)
    return [[], one, list(one), pick(3, sorted({0, k - 1})), pick(9), pick(16), pick(k if k <= 37 else 2), []]


def entry_list(rows, seed):
    """(stripe, index) entries of every stripe, shuffled with a fixed seed."""
    ent = [(z, j) for z, lst in enumerate(rows) for j in lst]
    order = np.random.default_rng(seed).permutation(len(ent))
    return [ent[i][0] for i in order], [ent[i][1] for i in order]


_cases = {}


def case(bits, k, p, S):
    """Old slab, the entry list, the new rows and the expected slab for a geometry
    and size: computed once, shared by the tests, never written."""
    key = (bits, k, p, S)
    if key in _cases:
        return _cases[key]
    seed = bits * 7919 + k * 131 + p * 17 + S
    rng = np.random.default_rng(seed)
    old = np.empty((NS, k + p, S), np.uint8)
    for z in range(NS):
        old[z, :k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
        old[z, k:] = orc.encode(bits, k, p, old[z, :k])
    rows = changed_rows(k, seed + 1)
    stripes, idx = entry_list(rows, seed + 2)
    new = rng.integers(0, 256, (len(idx), S), dtype=np.uint8)
    want = old.copy()
    for e, (z, j) in enumerate(zip(stripes, idx)):
        want[z, j] = new[e]
    for z in range(NS):
        if rows[z]:
            want[z, k:] = orc.encode(bits, k, p, want[z, :k])
    for a in (old, new, want):
        a.setflags(write=False)
    _cases[key] = (old, rows, stripes, idx, new, want)
    return _cases[key]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared references are read-only


def padded_slab(old):
    """The slab as a padded view: row_stride = S + 64, backing prefilled with 0xA5."""
    ns, total, S = old.shape
    backing = torch.full((ns, total, S + PAD), 0xA5, dtype=torch.uint8, device=DEV)
    slab = backing[:, :, :S]
    slab.copy_(dev(old))
    assert slab.stride(1) == S + PAD
    return backing, slab


def test_list_shape():
    """The list the other tests run has the shapes they are meant to cover."""
    k = 128
    _, rows, stripes, idx, _, _ = case(16, k, 32, 64)
    assert [len(r) for r in rows] == [0, 1, 1, 3, 9, 16, 2, 0]
    assert rows[1] == rows[2] and 0 in rows[3] and k - 1 in rows[3]
    assert [len(r) for r in changed_rows(37, 1)] == [0, 1, 1, 3, 9, 16, 37, 0]
    assert [len(r) for r in changed_rows(2, 1)] == [0, 1, 1, 2, 2, 2, 2, 0]
    for z in (4, 5):  # no stripe's entries are adjacent or sorted
        at = [e for e, zz in enumerate(stripes) if zz == z]
        assert at[-1] - at[0] >= len(at)
        assert [idx[e] for e in at] != sorted(idx[e] for e in at)


@pytest.mark.parametrize("width", [0, 1])
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("bits,k,p", GEOMS)
def test_update_list_matches_oracle(paths, bits, k, p, S, width):
    """unit_width 0: the 32-byte (GF(2^8): 16-byte) units a large grid selects; 1: the narrow ones."""
    paths("unit_width", width)
    old, rows, stripes, idx, new_np, want = case(bits, k, p, S)
    backing, slab = padded_slab(old)
    new = dev(new_np)
    c = rs.ReedSolomon(k, p, bits)
    c.update_dev_batch_list(slab, stripes, idx, new)
    torch.cuda.synchronize()
    got = backing.cpu().numpy()
    for z in range(NS):
        assert np.array_equal(got[z, :k, :S], want[z, :k]), f"stripe {z}: data rows ({bits} {k}+{p} S={S})"
        assert np.array_equal(got[z, k:, :S], want[z, k:]), f"stripe {z}: parity rows ({bits} {k}+{p} S={S})"
    for z in (0, 7):
        assert np.array_equal(got[z, :, :S], old[z]), f"stripe {z} is not named and was written"
    assert (got[:, :, S:] == 0xA5).all(), "padding bytes written"
    assert np.array_equal(new.cpu().numpy(), new_np), "new rows written"
    paths("unit_width", -1)
    assert c.verify_dev_batch(slab)


@pytest.mark.parametrize("null_stream", [False, True])
def test_update_list_is_stream_ordered(null_stream):
    """new = mask ^ 0x5A is computed by a torch op on the stream and the update is
    queued right behind it: no synchronise in between."""
    bits, k, p, S = 16, 128, 32, 4096 + 64
    old, rows, stripes, idx, new_np, want = case(bits, k, p, S)
    backing, slab = padded_slab(old)
    dmask = dev(new_np ^ 0x5A)
    c = rs.ReedSolomon(k, p, bits)
    torch.cuda.synchronize()
    st = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    if null_stream:
        assert rs.codec._stream_handle(st) == rs.codec.RS_NULL_STREAM
    with torch.cuda.stream(st):
        new = torch.bitwise_xor(dmask, 0x5A)
        c.update_dev_batch_list(slab, stripes, idx, new, stream=st)
    st.synchronize()
    assert np.array_equal(slab.cpu().numpy(), want)


def test_round_trip_restores_parity():
    """A -> B -> A: the second call's new rows are the first call's old ones."""
    bits, k, p, S = 16, 37, 9, 192
    old, rows, stripes, idx, new_np, want = case(bits, k, p, S)
    backing, slab = padded_slab(old)
    c = rs.ReedSolomon(k, p, bits)
    c.update_dev_batch_list(slab, stripes, idx, dev(new_np))
    torch.cuda.synchronize()
    assert np.array_equal(slab.cpu().numpy(), want) and not np.array_equal(want, old)
    back = np.stack([old[z, j] for z, j in zip(stripes, idx)])
    c.update_dev_batch_list(slab, stripes, idx, dev(back))
    torch.cuda.synchronize()
    assert np.array_equal(slab.cpu().numpy(), old)
    assert (backing.cpu().numpy()[:, :, S:] == 0xA5).all()


def test_column_set_cache_eviction():
    """Six calls whose column sets do not contain one another, through the 4-set
    cache, then the first again: its set was evicted and is rebuilt."""
    bits, k, p, S = 16, 37, 9, 192
    old = case(bits, k, p, S)[0]
    backing, slab = padded_slab(old)
    c = rs.ReedSolomon(k, p, bits)
    rng = np.random.default_rng(2025)
    cur = np.array(old)
    sets = [[n, n + 6, n + 12] for n in range(6)]
    for cols in sets + [sets[0]]:
        stripes = [1, 6, 6, 3]
        idx = [cols[0], cols[1], cols[2], cols[0]]
        new_np = rng.integers(0, 256, (len(idx), S), dtype=np.uint8)
        c.update_dev_batch_list(slab, stripes, idx, dev(new_np))
        for e, (z, j) in enumerate(zip(stripes, idx)):
            cur[z, j] = new_np[e]
    torch.cuda.synchronize()
    for z in range(NS):
        cur[z, k:] = orc.encode(bits, k, p, cur[z, :k])
    assert np.array_equal(slab.cpu().numpy(), cur)


def test_several_passes():
    """12+32768: a column's tables take 3 MiB, so the 32 MiB table bound holds
    8 columns (a multiple of the group size) and ten distinct columns run as two passes (8 + 2).  Stripe 0
    changes ten rows (a group of 8 in the first pass, 2 in the second), stripe 1
    one row of each pass."""
    bits, k, p, S = 16, 12, 32768, 64
    rng = np.random.default_rng(12 + 32768)
    old = np.empty((2, k + p, S), np.uint8)
    for z in range(2):
        old[z, :k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
        old[z, k:] = orc.encode(bits, k, p, old[z, :k])
    ent = [(0, j) for j in range(10)] + [(1, 3), (1, 9)]
    order = rng.permutation(len(ent))
    stripes, idx = [ent[i][0] for i in order], [ent[i][1] for i in order]
    new_np = rng.integers(0, 256, (len(idx), S), dtype=np.uint8)
    want = old.copy()
    for e, (z, j) in enumerate(zip(stripes, idx)):
        want[z, j] = new_np[e]
    for z in range(2):
        want[z, k:] = orc.encode(bits, k, p, want[z, :k])
    backing, slab = padded_slab(old)
    c = rs.ReedSolomon(k, p, bits)
    c.update_dev_batch_list(slab, stripes, idx, dev(new_np))
    torch.cuda.synchronize()
    got = backing.cpu().numpy()
    assert np.array_equal(got[:, :, :S], want)
    assert (got[:, :, S:] == 0xA5).all(), "padding bytes written"


@pytest.mark.parametrize("bits,k,p", [(16, 128, 32), (8, 10, 4)])
def test_single_entry_equals_update_dev_batch(bits, k, p):
    """One entry, against rs_update_dev_batch with nstripes = 1 on a copy of the slab."""
    S, z, j = 4096 + 64, 5, k - 2
    old = case(bits, k, p, S)[0]
    _, slab = padded_slab(old)
    _, ref = padded_slab(old)
    row = dev(np.random.default_rng(k).integers(0, 256, (1, S), dtype=np.uint8))
    c = rs.ReedSolomon(k, p, bits)
    c.update_dev_batch_list(slab, [z], [j], row)
    c.update_dev_batch(ref[z:z + 1], [j], row.reshape(1, 1, S))
    torch.cuda.synchronize()
    assert torch.equal(slab, ref)
    assert not np.array_equal(slab[z].cpu().numpy(), old[z])
    want = np.array(old[z, :k])
    want[j] = row.cpu().numpy()[0]
    assert np.array_equal(slab[z, k:].cpu().numpy(), orc.encode(bits, k, p, want))
