"""GPU tests of the incremental parity update (rs_update_dev, rs_encode_idx_dev,
rs_update_dev_batch; stream_kernels.hip k_update) against the oracle: after an update
the parity rows must be, bit for bit, the oracle's encode of the new data.
"""
import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [64, 192, 4096 + 64]

# (bits, k, p, changed rows)
UPDATE_CASES = [
    (16, 128, 32, [0]),
    (16, 128, 32, [127]),
    (16, 128, 32, [5, 31, 32, 100]),
    (16, 128, 32, [3, 17, 31, 32, 33, 64, 95, 96, 127]),  # nine rows: more than one launch group
    (16, 37, 9, list(range(37))),
    (16, 3, 7, [1]),
    (16, 2, 1, [0, 1]),
    (16, 1, 1, [0]),
    (16, 300, 300, [0, 150, 299]),  # m = 512
    (8, 10, 4, [9, 2]),
    (8, 100, 28, [0, 31, 32, 64, 99]),
    (8, 128, 128, [127, 0, 77]),
]

_stripes = {}


def stripe(bits, k, p, S):
    """(old data, its oracle parity) for a geometry and size, computed once and never written."""
    key = (bits, k, p, S)
    if key not in _stripes:
        rng = np.random.default_rng(bits * 7919 + k * 131 + p * 17 + S)
        data = rng.integers(0, 256, (k, S), dtype=np.uint8)
        par = orc.encode(bits, k, p, data)
        data.setflags(write=False)
        par.setflags(write=False)
        _stripes[key] = (data, par)
    return _stripes[key]


def new_rows_for(bits, k, p, S, changed):
    rng = np.random.default_rng(S * 31 + len(changed) * 7 + changed[0] + bits)
    return {j: rng.integers(0, 256, S, dtype=np.uint8) for j in changed}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared references are read-only


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("bits,k,p,changed", UPDATE_CASES, ids=lambda v: str(v) if not isinstance(v, list) else f"t{len(v)}")
def test_update_dev_matches_oracle(bits, k, p, changed, S):
    old, par = stripe(bits, k, p, S)
    nr = new_rows_for(bits, k, p, S, changed)
    new = old.copy()
    for j, r in nr.items():
        new[j] = r
    want = orc.encode(bits, k, p, new)
    c = rs.ReedSolomon(k, p, bits)
    # separate allocations; only the changed data rows are handed over
    rows = [dev(old[j]) if j in nr else None for j in range(k)] + [dev(par[i]) for i in range(p)]
    new_rows = [dev(nr[j]) if j in nr else None for j in range(k)]
    c.update_dev(rows, new_rows)
    torch.cuda.synchronize()
    got = np.stack([rows[k + i].cpu().numpy() for i in range(p)])
    assert np.array_equal(got, want), f"parity differs from the oracle's encode of the new data ({bits} {k}+{p} S={S})"
    for j in changed:
        assert np.array_equal(rows[j].cpu().numpy(), old[j]), "old data row written"
        assert np.array_equal(new_rows[j].cpu().numpy(), nr[j]), "new data row written"
    full = [dev(new[j]) for j in range(k)] + rows[k:]
    assert c.verify_dev(full)


@pytest.mark.parametrize("bits,k,p", [(16, 128, 32), (16, 37, 9), (8, 10, 4)])
def test_encode_idx_dev_builds_the_encode(bits, k, p):
    S = 192
    data, want = stripe(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    parity = [torch.zeros(S, dtype=torch.uint8, device=DEV) for _ in range(p)]
    order = np.random.default_rng(k * 3 + p).permutation(k)
    rows = {int(j): dev(data[j]) for j in order}
    for j in order:
        c.encode_idx_dev(rows[int(j)], int(j), parity)
    torch.cuda.synchronize()
    got = np.stack([t.cpu().numpy() for t in parity])
    assert np.array_equal(got, want)
    for j in (0, k - 1):
        assert np.array_equal(rows[j].cpu().numpy(), data[j])


@pytest.mark.parametrize("bits,k,p", [(16, 128, 32), (8, 10, 4)])
def test_update_dev_batch_padded_view(bits, k, p):
    S, ns, pad = 192, 3, 64
    idx = [k - 1, 0, 7]
    rng = np.random.default_rng(k + p + bits)
    backing = torch.full((ns, k + p, S + pad), 0xA5, dtype=torch.uint8, device=DEV)
    slab = backing[:, :, :S]
    assert slab.stride(1) == S + pad
    old = rng.integers(0, 256, (ns, k, S), dtype=np.uint8)
    new_np = rng.integers(0, 256, (ns, len(idx), S), dtype=np.uint8)
    for z in range(ns):
        slab[z, :k] = dev(old[z])
        slab[z, k:] = dev(orc.encode(bits, k, p, old[z]))
    new = dev(new_np)
    c = rs.ReedSolomon(k, p, bits)
    c.update_dev_batch(slab, idx, new)
    torch.cuda.synchronize()
    got = backing.cpu().numpy()
    for z in range(ns):
        d = old[z].copy()
        for j, i in enumerate(idx):
            d[i] = new_np[z, j]
        assert np.array_equal(got[z, :k, :S], d), f"stripe {z}: data rows"
        assert np.array_equal(got[z, k:, :S], orc.encode(bits, k, p, d)), f"stripe {z}: parity rows"
    assert (got[:, :, S:] == 0xA5).all(), "padding bytes written"
    assert np.array_equal(new.cpu().numpy(), new_np), "new rows written"
    assert c.verify_dev_batch(slab)


@pytest.mark.parametrize("null_stream", [False, True])
def test_update_is_stream_ordered(null_stream):
    """new = old ^ mask is computed by a torch op on the stream and the update
    is queued right behind it: no synchronise in between."""
    bits, k, p, S = 16, 128, 32, 4096 + 64
    changed = [2, 64]
    old, par = stripe(bits, k, p, S)
    rng = np.random.default_rng(99 + null_stream)
    mask = rng.integers(1, 256, (len(changed), S), dtype=np.uint8)
    new = np.array(old)
    for n, j in enumerate(changed):
        new[j] = old[j] ^ mask[n]
    want = orc.encode(bits, k, p, new)
    c = rs.ReedSolomon(k, p, bits)
    rows = [dev(old[j]) if j in changed else None for j in range(k)] + [dev(par[i]) for i in range(p)]
    dmask = dev(mask)
    torch.cuda.synchronize()
    st = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    if null_stream:
        assert rs.codec._stream_handle(st) == rs.codec.RS_NULL_STREAM
    with torch.cuda.stream(st):
        new_rows = [None] * k
        for n, j in enumerate(changed):
            new_rows[j] = torch.bitwise_xor(rows[j], dmask[n])
        c.update_dev(rows, new_rows, stream=st)
    st.synchronize()
    got = np.stack([rows[k + i].cpu().numpy() for i in range(p)])
    assert np.array_equal(got, want)


def test_round_trip_restores_parity():
    bits, k, p, S = 16, 128, 32, 192
    a, par = stripe(bits, k, p, S)
    changed = [1, 40, 41, 90, 127]
    nr = new_rows_for(bits, k, p, S, changed)
    c = rs.ReedSolomon(k, p, bits)
    prow = [dev(par[i]) for i in range(p)]
    ra = {j: dev(a[j]) for j in changed}
    rb = {j: dev(nr[j]) for j in changed}
    c.update_dev([ra.get(j) for j in range(k)] + prow, [rb.get(j) for j in range(k)])
    torch.cuda.synchronize()
    mid = np.stack([t.cpu().numpy() for t in prow])
    assert not np.array_equal(mid, par)
    c.update_dev([rb.get(j) for j in range(k)] + prow, [ra.get(j) for j in range(k)])
    torch.cuda.synchronize()
    assert np.array_equal(np.stack([t.cpu().numpy() for t in prow]), par)


def test_plan_cache_eviction():
    """20 different index lists on one codec, then the first again: past the
    16-entry table cache, so its tables are rebuilt."""
    bits, k, p, S = 16, 37, 9, 192
    old, par = stripe(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    rng = np.random.default_rng(2024)
    lists = [[n, (n + 11) % k] for n in range(20)]
    cur = np.array(old)
    drow = [dev(cur[j]) for j in range(k)]
    prow = [dev(par[i]) for i in range(p)]
    for lst in lists + [lists[0]]:
        nr = {j: rng.integers(0, 256, S, dtype=np.uint8) for j in lst}
        new_rows = [dev(nr[j]) if j in nr else None for j in range(k)]
        c.update_dev([drow[j] if j in nr else None for j in range(k)] + prow, new_rows)
        for j in lst:
            cur[j] = nr[j]
            drow[j] = new_rows[j]
    torch.cuda.synchronize()
    got = np.stack([t.cpu().numpy() for t in prow])
    assert np.array_equal(got, orc.encode(bits, k, p, cur))
