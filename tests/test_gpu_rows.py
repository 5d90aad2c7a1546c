"""GPU tests of the selective reconstruct (rs_reconstruct_rows_dev,
rs_reconstruct_rows_dev_batch, rs_reconstruct_rows) under both tiers: the
restricted transform (rows_direct 0) and the direct decode kernel (rows_direct
1, stream_kernels.hip k_decode_rows).  The wanted rows must be, bit for bit, what the
oracle's Reconstruct puts there for the same present rows, and no other byte
may change.
"""
import numpy as np
import pytest
import torch

import reedsolomon16_amd as rs
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5
GATE_N = 2048  # the direct tier serves decode transforms up to this many rows

# (bits, k, p, sizes)
GEOMS = [
    (16, 128, 32, [64, 192, 4160]),
    (16, 37, 9, [64, 192, 4160]),
    (16, 3, 7, [64, 192, 4160]),
    (16, 2, 1, [64, 192, 4160]),
    (16, 1, 1, [64, 192, 4160]),
    (16, 300, 300, [64, 192, 4160]),
    (16, 1024, 256, [64, 192]),   # n = 2048: the last size the direct tier serves
    (16, 2100, 100, [64]),        # n = 4096: beyond the gate, the restricted transform only
    (8, 10, 4, [64, 192, 4160]),
    (8, 100, 28, [64, 192, 4160]),
    (8, 128, 128, [64, 192, 4160]),
]
CASES = [(b, k, p, S) for b, k, p, sizes in GEOMS for S in sizes]


def ceil_pow2(x):
    return 1 << max(x - 1, 0).bit_length()


def gate_admits(k, p):
    return ceil_pow2(ceil_pow2(p) + k) <= GATE_N


def tiers(k, p):
    return [0, 1] if gate_admits(k, p) else [0]


_stripes = {}
_oracle = {}


def stripe(bits, k, p, S, tamper=None):
    """An encoded stripe (k+p rows), computed once and never written; tamper:
    index of a row replaced by random bytes, so the rows are no codeword."""
    key = (bits, k, p, S, tamper)
    if key not in _stripes:
        rng = np.random.default_rng(bits * 7919 + k * 131 + p * 17 + S)
        data = rng.integers(0, 256, (k, S), dtype=np.uint8)
        full = np.concatenate([data, orc.encode(bits, k, p, data)])
        if tamper is not None:
            full[tamper] ^= rng.integers(1, 256, S, dtype=np.uint8)  # every byte of the row changes
        full.setflags(write=False)
        _stripes[key] = full
    return _stripes[key]


def tamper_row(bits, k, p, present):
    """A row to tamper for a pattern: one of the rows the pattern has present,
    so the rows handed to the codec are inconsistent with each other."""
    rows = np.flatnonzero(present)
    row = int(rows[np.random.default_rng(bits + k * 3 + p * 5 + rows.size).integers(0, rows.size)])
    assert present[row]
    return row


def oracle_rows(bits, k, p, S, present, tamper=None):
    """{missing index: the oracle's Reconstruct of that row} for a pattern, computed once."""
    key = (bits, k, p, S, tamper, present.tobytes())
    if key not in _oracle:
        full = stripe(bits, k, p, S, tamper)
        lst = [np.array(full[i]) if present[i] else None for i in range(k + p)]
        e, out = orc.Oracle(bits, k, p).reconstruct(lst, recover_all=True)
        assert e == 0, e
        _oracle[key] = {i: out[i] for i in range(k + p) if not present[i]}
    return _oracle[key]


def patterns(bits, k, p):
    """name -> (present, required).  Missing rows are drawn once per geometry."""
    rng = np.random.default_rng(bits * 31 + k * 7 + p)
    total = k + p
    out = {}

    def flags(idx):
        f = np.zeros(total, bool)
        f[list(idx)] = True
        return f

    d, q = int(rng.integers(0, k)), k + int(rng.integers(0, p))
    out["one_data"] = (~flags([d]), flags([d]))
    if p == 1:  # one row missing: the data row, or the parity row
        out["p_missing_data"] = (~flags([d]), flags([d]))
        out["p_missing_parity"] = (~flags([q]), flags([q]))
        mixed, three = [q], [q]
    else:  # p rows missing, a data row and a parity row among them
        rest = [i for i in range(total) if i not in (d, q)]
        others = sorted(rng.choice(rest, p - 2, replace=False).tolist())
        mixed, three = sorted([d, q] + others), [d, q] + others[:1]
        out["p_missing_data"] = (~flags(mixed), flags([d]))
        out["p_missing_parity"] = (~flags(mixed), flags([q]))
    out["mix_of_three"] = (~flags(mixed), flags(three))
    if len(mixed) >= 9:  # more than one launch group of the direct kernel
        out["nine"] = (~flags(mixed), flags(mixed[:4] + mixed[-5:]))
    out["all_missing"] = (~flags(mixed), np.ones(total, bool))  # flags on present rows are ignored
    out["present_only"] = (~flags(mixed), ~flags(mixed))        # nothing to rebuild
    return out


def dev_slab(full, present):
    """The stripe on the device with every missing row filled with FILL."""
    a = np.array(full)
    a[~present] = FILL
    return torch.from_numpy(a).to(DEV)


def expected(full, present, required, want_rows):
    a = np.array(full)
    a[~present] = FILL
    for i in np.flatnonzero(~present & required):
        a[i] = want_rows[int(i)]
    return a


def check_all_classes(paths, bits, k, p, S, tier, tamper=False, names=None):
    """tamper: every pattern runs on a stripe with one of ITS present rows tampered."""
    paths("rows_direct", tier)
    c = rs.ReedSolomon(k, p, bits)
    for name, (present, required) in patterns(bits, k, p).items():
        if names and name not in names:
            continue
        bad_row = tamper_row(bits, k, p, present) if tamper else None
        full = stripe(bits, k, p, S, bad_row)
        want = oracle_rows(bits, k, p, S, present, bad_row)
        if tamper:  # the tampered row is one the codec reads, and it changes what is rebuilt
            clean = oracle_rows(bits, k, p, S, present)
            assert present[bad_row]
            assert all(not np.array_equal(want[i], clean[i]) for i in np.flatnonzero(~present & required))
        slab = dev_slab(full, present)
        c.reconstruct_rows_dev(slab, present, required)
        torch.cuda.synchronize()
        got = slab.cpu().numpy()
        exp = expected(full, present, required, want)
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert bad.size == 0, f"{bits} {k}+{p} S={S} tier {tier} {name}: rows {bad[:8]} differ"
        if name == "all_missing":  # equals reconstruct_dev's rows
            ref = dev_slab(full, present)
            c.set_reference_inversion_cache(False)
            c.reconstruct_dev(ref, present)
            torch.cuda.synchronize()
            assert torch.equal(ref, slab), f"{bits} {k}+{p} S={S} tier {tier}: differs from reconstruct_dev"
    c.close()


@pytest.mark.parametrize("bits,k,p,S,tier", [(b, k, p, S, t) for b, k, p, S in CASES for t in tiers(k, p)])
def test_rows_dev_matches_oracle(paths, bits, k, p, S, tier):
    check_all_classes(paths, bits, k, p, S, tier)


def test_beyond_the_gate_the_knob_changes_nothing(paths):
    """rows_direct 1 admits only n <= 2048: 2100+100 still runs the restricted transform."""
    check_all_classes(paths, 16, 2100, 100, 64, 1, names=("mix_of_three", "nine"))


@pytest.mark.parametrize("bits,k,p,S,tier", [(b, k, p, 192 if 192 in sizes else sizes[0], t)
                                             for b, k, p, sizes in GEOMS for t in tiers(k, p)])
def test_rows_dev_on_an_inconsistent_stripe(paths, bits, k, p, S, tier):
    """One present row tampered: the rebuilt rows still equal the oracle's,
    which pins the linear map (every present row, the pattern's locators)."""
    check_all_classes(paths, bits, k, p, S, tier, tamper=True,
                      names=("p_missing_data", "p_missing_parity", "mix_of_three", "nine"))


@pytest.mark.parametrize("bits,k,p", [(16, 128, 32), (8, 100, 28)])
def test_rows_dev_automatic_tier(paths, bits, k, p):
    check_all_classes(paths, bits, k, p, 192, -1)


@pytest.mark.parametrize("tier", [0, 1])
@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 4160), (8, 10, 4, 192), (16, 1024, 256, 64), (16, 37, 9, 64)])
def test_pointer_form_with_none_and_a_separate_output(paths, bits, k, p, S, tier):
    paths("rows_direct", tier)
    full = stripe(bits, k, p, S)
    present, required = patterns(bits, k, p)["mix_of_three"]
    want = oracle_rows(bits, k, p, S, present)
    c = rs.ReedSolomon(k, p, bits)
    src = [torch.from_numpy(np.array(full[i])).to(DEV) if present[i] else None for i in range(k + p)]
    rows = list(src)
    outs = {}
    for i in np.flatnonzero(~present & required):
        outs[int(i)] = rows[int(i)] = torch.full((S,), FILL, dtype=torch.uint8, device=DEV)
    assert any(r is None for r in rows) or p == 1
    c.reconstruct_rows_dev(rows, present, required)
    torch.cuda.synchronize()
    for i, t in outs.items():
        assert np.array_equal(t.cpu().numpy(), want[i]), f"row {i}"
    for i in np.flatnonzero(present):
        assert np.array_equal(src[int(i)].cpu().numpy(), full[i]), f"present row {i} written"
    c.close()


@pytest.mark.parametrize("bits,k,p,S,tier", [
    (b, k, p, S, t) for b, k, p, S in [(16, 128, 32, 192), (8, 100, 28, 4160), (16, 300, 300, 64), (16, 2100, 100, 64)]
    for t in tiers(k, p)])
def test_batch_on_a_padded_strided_view(paths, bits, k, p, S, tier):
    paths("rows_direct", tier)
    ns, total, PAD = 3, k + p, 0x5A
    present, required = patterns(bits, k, p)["mix_of_three"]
    c = rs.ReedSolomon(k, p, bits)
    big = torch.full((ns, total + 1, S + 64), PAD, dtype=torch.uint8, device=DEV)
    exp = np.full((ns, total + 1, S + 64), PAD, np.uint8)
    for z in range(ns):
        tamper = tamper_row(bits, k, p, present) if z == 1 else None  # one of the stripes is no codeword
        full = stripe(bits, k, p, S, tamper)
        big[z, :total, :S] = dev_slab(full, present)
        exp[z, :total, :S] = expected(full, present, required, oracle_rows(bits, k, p, S, present, tamper))
    c.reconstruct_rows_dev_batch(big[:, :total, :S], present, required)
    torch.cuda.synchronize()
    assert np.array_equal(big.cpu().numpy(), exp)
    c.close()


def test_multi_pass_route_is_restricted_too(paths):
    """lds_big 0 sends n = 4096 through the multi-pass kernels."""
    paths("lds_big", 0)
    check_all_classes(paths, 16, 2100, 100, 64, 0, names=("mix_of_three", "present_only"))


@pytest.mark.parametrize("tier", [0, 1])
@pytest.mark.parametrize("null_stream", [False, True], ids=["side", "null"])
def test_stream_order(paths, tier, null_stream):
    """The call is ordered on its stream: behind the copy that brings the rows
    in and ahead of the copy that takes them out, with no host wait between."""
    paths("rows_direct", tier)
    bits, k, p, S = 16, 128, 32, 4160
    full = stripe(bits, k, p, S)
    present, required = patterns(bits, k, p)["mix_of_three"]
    exp = expected(full, present, required, oracle_rows(bits, k, p, S, present))
    c = rs.ReedSolomon(k, p, bits)
    src = dev_slab(full, present)
    slab = torch.zeros_like(src)
    stream = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(3):
            slab.copy_(src, non_blocking=True)
            c.reconstruct_rows_dev(slab, present, required)
            got = slab.clone()
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), exp)
    c.close()


@pytest.mark.parametrize("tier", [0, 1])
def test_twenty_pairs_through_the_plan_caches(paths, tier):
    paths("rows_direct", tier)
    bits, k, p, S = 16, 37, 9, 192
    full = stripe(bits, k, p, S)
    c = rs.ReedSolomon(k, p, bits)
    rng = np.random.default_rng(20)
    pairs = []
    for j in range(20):
        present = np.ones(k + p, bool)
        present[rng.choice(k + p, 1 + j % p, replace=False)] = False
        required = np.zeros(k + p, bool)
        miss = np.flatnonzero(~present)
        required[miss[: 1 + j % 3]] = True
        pairs.append((present, required))
    for present, required in pairs + pairs[:4]:  # the first four were evicted by then
        slab = dev_slab(full, present)
        c.reconstruct_rows_dev(slab, present, required)
        torch.cuda.synchronize()
        assert np.array_equal(slab.cpu().numpy(), expected(full, present, required, oracle_rows(bits, k, p, S, present)))
    c.close()


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 4160), (8, 10, 4, 192), (16, 300, 300, 64)])
def test_host_rows(bits, k, p, S, multi, pinned):
    full = stripe(bits, k, p, S)
    present, required = patterns(bits, k, p)["mix_of_three"]
    want = oracle_rows(bits, k, p, S, present)
    c = rs.ReedSolomon(k, p, bits, devices=[0, 0, 0, 0]) if multi else rs.ReedSolomon(k, p, bits)

    def buf(src=None):
        b = rs.alloc_pinned(S) if pinned else np.empty(S, np.uint8)
        b[:] = FILL if src is None else src
        return b

    bufs = {int(i): buf() for i in np.flatnonzero(~present & required)}
    shards = [buf(full[i]) if present[i] else (rs.EmptyShard(bufs[i]) if i in bufs else None) for i in range(k + p)]
    out = c.reconstruct_rows(shards, required)
    for i in range(k + p):
        if present[i]:
            assert np.array_equal(out[i], full[i]), f"present row {i} written"
        elif required[i]:
            assert np.array_equal(out[i], want[i]), f"row {i}"
            assert np.array_equal(bufs[i], want[i]), f"row {i} did not land in its buffer"
        else:
            assert out[i] is None, f"unwanted row {i} came back"  # its len stays 0
    c.close()


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("bits,k,p,S", [(16, 128, 32, 192), (8, 10, 4, 64), (16, 300, 300, 64)])
def test_host_rows_lens(bits, k, p, S, multi):
    """rs_reconstruct_rows sets lens[i] = S for the rebuilt rows only: every
    missing row has a buffer here, and the unwanted ones keep len 0 and their bytes."""
    import ctypes as C

    from reedsolomon16_amd import _capi

    full = stripe(bits, k, p, S)
    present, required = patterns(bits, k, p)["mix_of_three"]
    want = oracle_rows(bits, k, p, S, present)
    total = k + p
    c = rs.ReedSolomon(k, p, bits, devices=[0, 0, 0, 0]) if multi else rs.ReedSolomon(k, p, bits)
    bufs = [np.array(full[i]) if present[i] else np.full(S, FILL, np.uint8) for i in range(total)]
    ptrs = (C.c_void_p * total)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * total)(*[S if present[i] else 0 for i in range(total)])
    req = (C.c_uint8 * total)(*[1 if x else 0 for x in required])
    assert _capi.lib().rs_reconstruct_rows(c._h, ptrs, lens, total, req) == 0
    rebuilt = ~present & required
    assert rebuilt.any() and (~present & ~required).any()
    assert list(lens) == [S if present[i] or rebuilt[i] else 0 for i in range(total)]
    for i in range(total):
        if rebuilt[i]:
            assert np.array_equal(bufs[i], want[i]), f"row {i}"
        elif present[i]:
            assert np.array_equal(bufs[i], full[i]), f"present row {i} written"
        else:
            assert (bufs[i] == FILL).all(), f"unwanted row {i} written"
    c.close()
